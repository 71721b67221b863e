// capi_plasticity.inc — the plasticity rule of a wgs_data (wgs_set_plasticity_model / wgs_get_plasticity_model) and everything that
// exists only under WGS_PLASTICITY_SNOW: the MODEL 4 instantiations of the fused G2P (g2p_body.inc; device_math.h snow_project), the
// field read-out and the two energy passes of the diagnostics with the hardened coefficients. The LAST part of capi.hip on purpose:
// the kernels below are instantiated here, behind every kernel that existed, so that each of those keeps its bytes and its place in
// the code object (tools/kernel_symbols_cmp.py; notes/round_31.md). The launch sites reach them by declaration: launch_g2p
// (host_substep.inc), wgs_read_particle_fields_device (capi_fields.inc), diag_enqueue (kernels_diag.h).
// The rule is a host-side choice of instantiation (wgs_data::plasticity), never a run-time branch in a kernel and not a field of Dev.

namespace {

// the corotated plastic ladder of launch_g2p under the snow rule: both bodies, every pass count, the dense and the regular register
// budget (launch_g2p_shape takes them from PL = true as for Drucker-Prager); no slab instantiation runs — the setter refuses slabs
void launch_g2p_snow(const Dev &dev, hipStream_t s, int side, uint32_t epoch, const G2pLaunch &p, const Mark &mark) {
    launch_g2p_model<D, 4, true>(dev, s, side, epoch, p, mark);
}

// (templates on the dimension although it is a constant of the library: a template is emitted where it is first launched — here, behind
// every other kernel —, a plain kernel where the file defines it in the order of all plain kernels: kernels_probe.h)
template <int DIM> __global__ __launch_bounds__(FIELD_THREADS) void k_particle_fields_snow(Dev d, int side, float *out) {
    constexpr bool SNOW = true;
#include "fields_body.inc"
}
void launch_particle_fields_snow(wgs_data *d, dim3 blocks, float *device_out) {
    hipLaunchKernelGGL(k_particle_fields_snow<D>, blocks, dim3(FIELD_THREADS), 0, d->stream, d->dev, d->side, device_out);
}

// (WGS_DIAG_ENERGY implies WGS_DIAG_PARTICLES, and the data carries plastic state: PART, ENERGY and `plastic` are all set whenever these
// run; the phase then comes from the plastic quads, never from the by-pid table)
template <int DIM, bool DIGEST> __global__ __launch_bounds__(256) void k_diag_pass1_snow(Dev d, int side, DiagAcc *acc) {
    constexpr bool SNOW = true, PART = true, ENERGY = true, plastic = true;
    const float *const phase_by_pid = nullptr;
#include "diag_pass1_body.inc"
}
template <int DIM> __global__ __launch_bounds__(256) void k_diag_pass2_snow(Dev d, int side, DiagAcc *acc) {
    constexpr bool SNOW = true, ENERGY = true;
#include "diag_pass2_body.inc"
}
void launch_diag_pass1_snow(wgs_data *d, bool digest, dim3 blocks, DiagAcc *acc) {
    if (digest) hipLaunchKernelGGL((k_diag_pass1_snow<D, true>), blocks, dim3(256), 0, d->stream, d->dev, d->side, acc);
    else hipLaunchKernelGGL((k_diag_pass1_snow<D, false>), blocks, dim3(256), 0, d->stream, d->dev, d->side, acc);
}
void launch_diag_pass2_snow(wgs_data *d, dim3 blocks, DiagAcc *acc) {
    hipLaunchKernelGGL(k_diag_pass2_snow<D>, blocks, dim3(256), 0, d->stream, d->dev, d->side, acc);
}

}  // namespace

extern "C" {

wgs_status wgs_set_plasticity_model(wgs_data *d, int32_t kind) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (kind != WGS_PLASTICITY_DRUCKER_PRAGER && kind != WGS_PLASTICITY_SNOW) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_plasticity_model: unknown kind (WGS_PLASTICITY_*)");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_plasticity_model: sharded wgs_data (the arrivals' kernel has no snow variant): single-domain data only");
    // (snow is the corotated stress with hardened coefficients; a table of per-particle models holds other models)
    if (kind == WGS_PLASTICITY_SNOW && (d->dev.model != WGS_MODEL_COROTATED || d->dev.pmodel[0]))
        return fail(WGS_ERR_UNSUPPORTED, "wgs_set_plasticity_model: WGS_PLASTICITY_SNOW is defined on WGS_MODEL_COROTATED (wgs_set_constitutive_model), without a table of per-particle models");
    d->plasticity = kind;   // (read when a substep, a field read-out or an energy sum is enqueued: stream-ordered like the other setters)
    return WGS_OK;
}

wgs_status wgs_get_plasticity_model(wgs_data *d, int32_t *out) {
    if (!d || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = d->plasticity;
    return WGS_OK;
}

}  // extern "C"
