// kernels_fluid.h — WGS_MODEL_FLUID (include/wgsparkl_hip.h): the kernel wgs_set_constitutive_model enqueues when the fluid is
// selected. The step itself is the fused G2P with MODEL = 2 (g2p_body.inc, arrivals_body.inc; the update is fluid_update,
// device_math.h). Included last by capi.hip, so that no kernel that existed before changes its place in the code object.
#pragma once

namespace {

// F of every slot of the current buffer -> diag(det F, 1[, 1]) (layout.h Dev::fluid_gamma on that form). mat_det of a value
// already in that form is its J bit for bit, so selecting the fluid twice, or on a restored checkpoint, changes nothing.
// Every slot up to the launch bound: on a slab that is its capacity (vacated and unused slots hold no particle; whatever
// their words are, nothing reads them).
__global__ void k_fluid_collapse(Dev d, int side) {
    using P = Pl<D>;
    float *buf = d.buf[side];
    const uint32_t npad = d.npad;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x) {
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
