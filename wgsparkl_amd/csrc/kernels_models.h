// kernels_models.h — per-particle constitutive models (include/wgsparkl_hip.h wgs_set_particle_models): the kernels of the setter and
// the reader. The step itself is the fused G2P with MODEL = 3 (g2p_body.inc), which carries the model byte of a particle from plane
// to plane beside its pid (layout.h Dev::pmodel). Included last by capi.hip, behind kernels_fluid.h: no kernel that existed before
// changes its place in the code object.
#pragma once

namespace {

// the caller's table (by persistent id) -> the plane of the current buffer (by slot), through the pid plane
__global__ void k_models_scatter(Dev d, int side, const uint8_t *by_pid) {
    const float *buf = d.buf[side];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x)
        d.pmodel[side][j] = by_pid[ldpid<D>(buf, d.npad, j)];
}

// ... and back; without a table (null planes) every particle has the data's model
__global__ void k_models_gather(Dev d, int side, uint8_t *by_pid) {
    const float *buf = d.buf[side];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x)
        by_pid[ldpid<D>(buf, d.npad, j)] = d.pmodel[side] ? d.pmodel[side][j] : (uint8_t)d.model;
}

// k_fluid_collapse (kernels_fluid.h) for the slots the table labels WGS_MODEL_FLUID: F -> diag(det F, 1[, 1]), the identity on a value
// already in that form. The other slots are not written. (A kernel of its own: k_fluid_collapse stays as it is.)
__global__ void k_fluid_collapse_masked(Dev d, int side) {
    using P = Pl<D>;
    float *buf = d.buf[side];
    const uint32_t npad = d.npad;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x) {
        if (d.pmodel[side][j] != WGS_MODEL_FLUID) continue;
        if constexpr (D == 3) {
            float4 xm = ldq(buf, npad, Pl<3>::XM, j), f2 = ldq(buf, npad, Pl<3>::F2, j);
            const float4 f0 = ldq(buf, npad, P::F0, j), f1 = ldq(buf, npad, Pl<3>::F1, j);
            const float F[9] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, d.uniform ? xm.w : f2.x};
            const float det = mat_det<3>(F);
            stq(buf, npad, P::F0, j, make_float4(det, 0.f, 0.f, 0.f));
            stq(buf, npad, Pl<3>::F1, j, make_float4(1.f, 0.f, 0.f, 0.f));
            if (d.uniform) {   // (F[8] rides in XM.w, the F2 quad is not maintained: layout.h)
                xm.w = 1.f;
                stq(buf, npad, Pl<3>::XM, j, xm);
            } else {
                f2.x = 1.f;
                stq(buf, npad, Pl<3>::F2, j, f2);
            }
        } else {
            const float4 f0 = ldq(buf, npad, P::F0, j);
            const float F[4] = {f0.x, f0.y, f0.z, f0.w};
            stq(buf, npad, P::F0, j, make_float4(mat_det<2>(F), 0.f, 0.f, 1.f));
        }
    }
}

}  // namespace
