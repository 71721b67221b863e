// kernels_emit.h — particles added at run time (include/wgsparkl_hip_emit.h): ONE device function that packs a particle record into a
// slot of the current buffer — what pack_slot / stage_particles / the uploads and the conversions to the uniform layouts do on the host
// at creation (capi_lifecycle.inc), in every layout —, and the two kernels that run it: k_append over records the caller handed over,
// k_emit over one batch of one emitter, the record built in registers from the emitter argument. One thread per new particle, plain
// vector stores; every bound is a launch argument (the host knows the particle count of single-domain data), never a device counter.
// Included last by capi.hip: no kernel that existed changes its place in the code object. The launches are in capi_emit.inc.
#pragma once

namespace {

// What the pack needs besides Dev, the same for every particle of a launch.
struct PackArgs {
    int side;              // the current buffer
    uint32_t stamp;        // cdf stamp of the new slots: the number of the last finished substep — 0 on new data, which is what creation
                           // leaves —, so that the record's cdf counts as that substep's, exactly as a record handed to wgs_data_create does
    float default_dp[6];   // DruckerPrager::new(-1, -1): the parameters of a particle without plasticity (capi_lifecycle.inc default_dp_params)
    float *s_radius, *s_dp, *s_phase;   // the by-pid tables of the handle (wgs_data::static_*)
    uint32_t *s_flags;
};

// Particle record `q` with position `x` -> slot j of the current buffer, persistent id `pid`; `model`: its WGS_MODEL_* (the table's byte,
// or the data's model). The device twin of pack_slot, quad by quad in the words of layout.h's table, then what the layouts add:
//   uniform material (3D): F[8] in XM.w (k_to_uniform);
//   uni_dp 1 / 2: the shared quads DP0 and DP2 in BOTH ping-pong buffers (to_uniform_layouts), mode 2: DP1 = (st0, st1, st2, phase);
//   WGS_MODEL_FLUID: F = diag(det F, 1[, 1]) (k_fluid_collapse: the same mat_det of the same floats);
//   the pid plane, the cdf stamp, the model planes of both sides, the by-pid tables.
template <int DIM>
__device__ __forceinline__ void pack_particle(const Dev &d, const PackArgs &a, uint32_t j, uint32_t pid, const wgs_particle &q, const float *x, uint32_t model) {
    using L = Pl<DIM>;
    float *buf = d.buf[a.side], *other = d.buf[a.side ^ 1];
    const uint32_t npad = d.npad;
    const wgs_particle_dynamics &dy = q.dynamics;
    const float *v = dy.velocity, *C = dy.affine, *nrm = dy.cdf.normal, *rvel = dy.cdf.rigid_vel;
    const float aff = __uint_as_float(dy.cdf.affinity);
    float F[DIM * DIM];
#pragma unroll
    for (int k = 0; k < DIM * DIM; k++) F[k] = dy.def_grad[k];
    const bool fluid = model == (uint32_t)WGS_MODEL_FLUID;
    const float det = mat_det<DIM>(F);
    if constexpr (DIM == 3) {
        const float f8 = fluid ? 1.f : F[m9(8)];
        stq(buf, npad, L::XM, j, make_float4(x[0], x[1], x[DIM - 1], d.uniform ? f8 : dy.mass));
        stq(buf, npad, L::CV0, j, make_float4(C[0], C[1], C[2], C[3]));
        stq(buf, npad, Pl<3>::CV1, j, make_float4(C[m9(4)], C[m9(5)], C[m9(6)], C[m9(7)]));
        stq(buf, npad, L::CV2, j, make_float4(C[m9(8)], v[0], v[1], v[DIM - 1]));
        stq(buf, npad, L::F0, j, fluid ? make_float4(det, 0.f, 0.f, 0.f) : make_float4(F[0], F[1], F[2], F[3]));
        stq(buf, npad, Pl<3>::F1, j, fluid ? make_float4(1.f, 0.f, 0.f, 0.f) : make_float4(F[m9(4)], F[m9(5)], F[m9(6)], F[m9(7)]));
        // (uniform material: the quad is not maintained by the step; it holds what the upload left, as at creation)
        stq(buf, npad, Pl<3>::F2, j, make_float4(d.uniform ? F[m9(8)] : f8, dy.init_volume, q.model.lambda, q.model.mu));
        stq(buf, npad, L::CDF0, j, make_float4(nrm[0], nrm[1], nrm[DIM - 1], dy.cdf.signed_distance));
        stq(buf, npad, L::CDF1, j, make_float4(rvel[0], rvel[1], rvel[DIM - 1], aff));
    } else {
        stq(buf, npad, L::XM, j, make_float4(x[0], x[1], dy.mass, dy.init_volume));
        stq(buf, npad, L::CV0, j, make_float4(C[0], C[1], C[2], C[3]));
        stq(buf, npad, L::CV2, j, make_float4(v[0], v[1], q.model.lambda, q.model.mu));
        stq(buf, npad, L::F0, j, fluid ? make_float4(det, 0.f, 0.f, 1.f) : make_float4(F[0], F[1], F[2], F[3]));
        stq(buf, npad, L::CDF0, j, make_float4(nrm[0], nrm[1], dy.cdf.signed_distance, aff));
        stq(buf, npad, L::CDF1, j, make_float4(rvel[0], rvel[1], 0.f, 0.f));
    }
    // plasticity parameters, plastic state {1, 1, 0} and phase (stage_particles)
    const bool has_pl = q.has_plasticity != 0u, has_ph = q.has_phase != 0u;
    const float dp0 = has_pl ? q.plasticity.h0 : a.default_dp[0], dp1 = has_pl ? q.plasticity.h1 : a.default_dp[1],
                dp2 = has_pl ? q.plasticity.h2 : a.default_dp[2], dp3 = has_pl ? q.plasticity.h3 : a.default_dp[3],
                dp4 = has_pl ? q.plasticity.lambda : a.default_dp[4], dp5 = has_pl ? q.plasticity.mu : a.default_dp[5];
    const float phase = has_ph ? q.phase.phase : 0.0f, max_stretch = has_ph ? q.phase.max_stretch : -1.0f;
    const float4 q0 = make_float4(dp0, dp1, dp2, dp3), q2 = make_float4(0.0f, phase, max_stretch, 0.f);
    stq(buf, npad, L::DP0, j, q0);
    stq(buf, npad, L::DP1, j, d.uni_dp == 2u ? make_float4(1.0f, 1.0f, 0.0f, phase) : make_float4(dp4, dp5, 1.0f, 1.0f));
    stq(buf, npad, L::DP2, j, q2);
    if (d.uni_dp != 0u) {   // (the quads the plastic step neither reads nor rewrites stand in both buffers for every slot: layout.h Dev::uni_dp)
        stq(other, npad, L::DP0, j, q0);
        stq(other, npad, L::DP2, j, q2);
    }
    stpid<DIM>(buf, npad, j, pid);
    ststamp<DIM>(buf, npad, j, a.stamp);
    if (d.pmodel[0]) {
        stmodel(d.pmodel[a.side], j, model);
        stmodel(d.pmodel[a.side ^ 1], j, model);
    }
    a.s_radius[pid] = dy.init_radius;
    float *sdp = a.s_dp + (size_t)pid * 6;
    sdp[0] = dp0; sdp[1] = dp1; sdp[2] = dp2; sdp[3] = dp3; sdp[4] = dp4; sdp[5] = dp5;
    a.s_phase[(size_t)pid * 2] = phase;
    a.s_phase[(size_t)pid * 2 + 1] = max_stretch;
    a.s_flags[pid] = (has_pl ? 1u : 0u) | (has_ph ? 2u : 0u);
}

// k records staged on the device -> slots [first, first + k) of the current buffer, ids [first, first + k). `models`: a byte per record, or
// null: the data's model (read only while the data carries a table: capi_emit.inc passes null otherwise).
template <int DIM> __global__ void k_append(Dev d, PackArgs a, uint32_t first, uint32_t k, const wgs_particle *records, const uint8_t *models) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const wgs_particle &q = records[t];
    float x[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) x[c] = q.position[c];
    pack_particle<DIM>(d, a, first + t, first + t, q, x, models ? (uint32_t)models[t] : (uint32_t)d.model);
}

// Batch `batch` of emitter `e_index` -> slots [first, first + total), total = prod(count): the lattice and the jitter of
// include/wgsparkl_hip_emit.h, every rounding a statement of its own (-ffp-contract=on fuses inside one expression only).
template <int DIM> __global__ void k_emit(Dev d, PackArgs a, uint32_t first, uint32_t total, wgs_emitter e, uint32_t e_index, uint32_t batch, uint32_t model) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint32_t i[3] = {t % e.count[0], t / e.count[0], 0u};
    if constexpr (DIM == 3) {
        i[2] = i[1] / e.count[1];
        i[1] = i[1] % e.count[1];
    }
    const uint32_t batch_hash = wgs_lowbias32(batch * 0x9E3779B9u + e_index);
    const float js = e.jitter * e.spacing;
    float x[DIM];
#pragma unroll
    for (int c = 0; c < DIM; c++) {
        const uint32_t hash = wgs_lowbias32(e.seed ^ batch_hash ^ wgs_lowbias32(t * (uint32_t)DIM + (uint32_t)c));
        const float r = (float)(hash >> 8);
        const float r01 = r * 5.9604644775390625e-8f;   // 2^-24: exact
        const float u = r01 - 0.5f;                      // exact
        const float cell = (float)i[c] + 0.5f;
        const float off = cell * e.spacing;
        const float at = e.lo[c] + off;
        const float jit = js * u;
        x[c] = at + jit;
    }
    pack_particle<DIM>(d, a, first + t, first + t, e.proto, x, model);
}

}  // namespace
