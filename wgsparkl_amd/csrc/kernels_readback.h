// kernels_readback.h — device code of the entry points that move particle and grid state out of (and the plastic state
// back into) the packed layout of layout.h: the readers of capi_io.inc, the checkpoint restore and the render hand-off.
// Kernels and their device helpers only; the entry points that launch them are in capi_io.inc.
#pragma once

namespace {

struct ParticleOffsets {  // word offsets inside wgs_particle
    uint32_t stride, pos, vel, F, C, nrm, rvel, dist, aff, vol, rad, mass, lam, mu, has_pl, dp, has_ph, phase;
};

// Unpacked view of one particle slot (quad layout of layout.h).
struct Unpacked {
    float x[D], v[D], F[DD], C[DD], mass, vol, lam, mu;
    float nrm[D], rvel[D], dist;
    uint32_t aff;
    float dp[6], st[3], phase[2];
};

// index into a 3x3 matrix; the 3D branch below is parsed (never run) in the 2D library too
[[maybe_unused]] constexpr int m9(int k) { return DD == 9 ? k : 0; }

template <int DIM> __device__ inline void unpack_slot(const float *in, uint32_t npad, uint32_t j, bool plastic, bool cpic_in, uint32_t cdf_epoch, Unpacked &u) {
    // cdf quads are valid only if stamped with the epoch of the last substep (0 = echo the input)
    const bool cpic = cpic_in && (cdf_epoch == 0u || ldstamp<DIM>(in, npad, j) == cdf_epoch);
    using P = Pl<DIM>;
    if constexpr (DIM == 3) {
        const float4 xm = ldq(in, npad, P::XM, j), c0 = ldq(in, npad, P::CV0, j), c1 = ldq(in, npad, P::CV1, j),
                     c2 = ldq(in, npad, P::CV2, j), f0 = ldq(in, npad, P::F0, j), f1 = ldq(in, npad, P::F1, j),
                     f2 = ldq(in, npad, P::F2, j);
        u.x[0] = xm.x; u.x[1] = xm.y; u.x[D - 1] = xm.z; u.mass = xm.w;  // (uniform-material mode: fixed up by the caller)
        u.C[0] = c0.x; u.C[1] = c0.y; u.C[2] = c0.z; u.C[3] = c0.w;
        u.C[m9(4)] = c1.x; u.C[m9(5)] = c1.y; u.C[m9(6)] = c1.z; u.C[m9(7)] = c1.w; u.C[m9(8)] = c2.x;
        u.v[0] = c2.y; u.v[1] = c2.z; u.v[D - 1] = c2.w;
        u.F[0] = f0.x; u.F[1] = f0.y; u.F[2] = f0.z; u.F[3] = f0.w;
        u.F[m9(4)] = f1.x; u.F[m9(5)] = f1.y; u.F[m9(6)] = f1.z; u.F[m9(7)] = f1.w; u.F[m9(8)] = f2.x;
        u.vol = f2.y; u.lam = f2.z; u.mu = f2.w;
    } else {
        const float4 xm = ldq(in, npad, P::XM, j), c0 = ldq(in, npad, P::CV0, j), vl = ldq(in, npad, P::CV2, j),
                     f0 = ldq(in, npad, P::F0, j);
        u.x[0] = xm.x; u.x[1] = xm.y; u.mass = xm.z; u.vol = xm.w;
        u.C[0] = c0.x; u.C[1] = c0.y; u.C[2] = c0.z; u.C[3] = c0.w;
        u.v[0] = vl.x; u.v[1] = vl.y; u.lam = vl.z; u.mu = vl.w;
        u.F[0] = f0.x; u.F[1] = f0.y; u.F[2] = f0.z; u.F[3] = f0.w;
    }
    for (int k = 0; k < D; k++) { u.nrm[k] = 0.f; u.rvel[k] = 0.f; }
    u.dist = 0.f;
    u.aff = 0u;
    if (cpic) {
        const float4 a = ldq(in, npad, P::CDF0, j), b = ldq(in, npad, P::CDF1, j);
        u.nrm[0] = a.x; u.nrm[1] = a.y; u.rvel[0] = b.x; u.rvel[1] = b.y;
        if constexpr (DIM == 3) { u.nrm[D - 1] = a.z; u.dist = a.w; u.rvel[D - 1] = b.z; u.aff = __float_as_uint(b.w); }
        else { u.dist = a.z; u.aff = __float_as_uint(a.w); }
    }
    if (plastic) {
        const float4 d0 = ldq(in, npad, P::DP0, j), d1 = ldq(in, npad, P::DP1, j), d2 = ldq(in, npad, P::DP2, j);
        u.dp[0] = d0.x; u.dp[1] = d0.y; u.dp[2] = d0.z; u.dp[3] = d0.w; u.dp[4] = d1.x; u.dp[5] = d1.y;
        u.st[0] = d1.z; u.st[1] = d1.w; u.st[2] = d2.x; u.phase[0] = d2.y; u.phase[1] = d2.z;
    }
}

// uniform-material mode (layout.h): XM.w holds F[8], the four constants are kernel arguments
template <int DIM> __device__ inline void fix_uniform(const Dev &d, Unpacked &u) {
    if constexpr (DIM == 3) {
        if (d.uniform) {
            u.F[m9(8)] = u.mass;
            u.mass = d.uni_mass; u.vol = d.uni_vol; u.lam = d.uni_lambda; u.mu = d.uni_mu;
        }
    }
    // uniform plasticity parameters (layout.h Dev::uni_dp): in mode 2 DP1 holds (st0, st1, st2, phase) — unpack_slot read it as
    // (dp4, dp5, st0, st1) — and DP2 is not kept up to date
    if (d.uni_dp == 2u) {
        const float s0 = u.dp[4], s1 = u.dp[5], s2 = u.st[0], ph = u.st[1];
        u.st[0] = s0; u.st[1] = s1; u.st[2] = s2;
        u.phase[0] = ph; u.phase[1] = d.uni_max_stretch;
    }
    if (d.uni_dp != 0u)
        for (int k = 0; k < (d.uni_dp == 2u ? 6 : 4); k++) u.dp[k] = d.uni_dpv[k];
}

// general layout -> uniform-material layout: F[8] takes the place of the mass in XM.w
// `check`: the caller ASSERTED the constants (wgs_set_uniform_material on sharded data): a particle that carries other
// values would silently lose them, so every particle is compared bit for bit first and a mismatch is reported
// (ERRBIT_MATERIAL -> the next wgs_sync).
__global__ void k_to_uniform(Dev d, int side, int check) {
    if constexpr (D == 3) {
        float *buf = d.buf[side];
        const uint32_t n = num_slots(d);
        for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
            float4 xm = ldq(buf, d.npad, Pl<3>::XM, j);
            const float4 f2 = ldq(buf, d.npad, Pl<3>::F2, j);
            if (check && (__float_as_uint(xm.w) != __float_as_uint(d.uni_mass) || __float_as_uint(f2.y) != __float_as_uint(d.uni_vol) ||
                          __float_as_uint(f2.z) != __float_as_uint(d.uni_lambda) || __float_as_uint(f2.w) != __float_as_uint(d.uni_mu)))
                atomicOr(&d.counters[CTR_ERRORS], ERRBIT_MATERIAL);
            xm.w = f2.x;
            stq(buf, d.npad, Pl<3>::XM, j, xm);
        }
    }
}

__global__ void k_export_particles(Dev d, int side, ParticleOffsets o, bool plastic, bool cpic, uint32_t cdf_epoch, const float *s_radius,
                                   const float *s_dp, const float *s_phase, const uint32_t *s_flags, float *out,
                                   float *plastic_out) {
    const float *in = d.buf[side];
    const uint32_t npad = d.npad;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x) {
        const uint32_t pid = ldpid<D>(in, npad, j);
        Unpacked u;
        unpack_slot<D>(in, npad, j, plastic, cpic, cdf_epoch, u);
        fix_uniform<D>(d, u);
        float *r = out + (size_t)pid * o.stride;
        for (int k = 0; k < D; k++) {
            r[o.pos + k] = u.x[k];
            r[o.vel + k] = u.v[k];
            r[o.nrm + k] = u.nrm[k];
            r[o.rvel + k] = u.rvel[k];
        }
        for (int k = 0; k < DD; k++) {
            r[o.F + k] = u.F[k];
            r[o.C + k] = u.C[k];
        }
        r[o.dist] = u.dist;
        r[o.aff] = __uint_as_float(u.aff);
        r[o.vol] = u.vol;
        r[o.rad] = s_radius[pid];
        r[o.mass] = u.mass;
        r[o.lam] = u.lam;
        r[o.mu] = u.mu;
        const uint32_t fl = s_flags[pid];
        r[o.has_pl] = __uint_as_float(fl & 1u);
        r[o.has_ph] = __uint_as_float((fl >> 1) & 1u);
        for (int k = 0; k < 6; k++) r[o.dp + k] = s_dp[(size_t)pid * 6 + k];
        r[o.phase] = plastic ? u.phase[0] : s_phase[(size_t)pid * 2];
        r[o.phase + 1] = plastic ? u.phase[1] : s_phase[(size_t)pid * 2 + 1];
        if (plastic_out)
            for (int k = 0; k < 3; k++) plastic_out[(size_t)pid * 3 + k] = plastic ? u.st[k] : (k < 2 ? 1.f : 0.f);
    }
}

// checkpoint restore: Drucker-Prager plastic state by persistent particle id (models/drucker_prager.wgsl:18-23)
__global__ void k_import_plastic_state(Dev d, int side, const float *states) {
    using P = Pl<D>;
    float *buf = d.buf[side];
    const uint32_t npad = d.npad;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < num_slots(d); j += gridDim.x * blockDim.x) {
        const uint32_t pid = ldpid<D>(buf, npad, j);
        if (pid == 0xffffffffu) continue;  // vacated slot of a sharded run
        const float *st = states + (size_t)pid * 3;
        float4 q1 = ldq(buf, npad, P::DP1, j), q2 = ldq(buf, npad, P::DP2, j);
        if (d.uni_dp == 2u) {   // (the state is one quad: layout.h)
            q1.x = st[0];
            q1.y = st[1];
            q1.z = st[2];
        } else {
            q1.z = st[0];
            q1.w = st[1];
            q2.x = st[2];
        }
        stq(buf, npad, P::DP1, j, q1);
        stq(buf, npad, P::DP2, j, q2);
    }
}

// Render hand-off: src_testbed/prep_vertex_buffer{2,3}d.wgsl `main`. Instance i = particle i of the
// caller's order; base_color is read from the instance record, everything else is written.
__global__ void k_prep_instances(Dev d, int side, uint32_t mode, bool cpic, uint32_t cdf_epoch, float *inst) {
    const float *in = d.buf[side];
    const uint32_t npad = d.npad;
    const float h = d.h, dt = d.sp->dt;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x) {
        const uint32_t pid = ldpid<D>(in, npad, j);
        Unpacked u;
        unpack_slot<D>(in, npad, j, false, cpic, cdf_epoch, u);
        fix_uniform<D>(d, u);
        float *r = inst + (size_t)pid * 24;
        // deformation: mat3x3 as three padded columns (instancing3d.rs:66-74); 2D embeds F in the xy block
        float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        // (the particle's own model where the data carries a table: layout.h Dev::pmodel)
        if ((d.pmodel[side] ? (int)d.pmodel[side][j] : d.model) == WGS_MODEL_FLUID) {   // F holds diag(J, 1[, 1]) (layout.h): drawn as the isotropic deformation of that volume ratio
            const float s = D == 3 ? cbrtf(u.F[0]) : sqrtf(u.F[0]);
            for (int k = 0; k < DD; k++) u.F[k] = 0.f;
            for (int k = 0; k < D; k++) u.F[k * D + k] = s;
        }
        for (int col = 0; col < D; col++)
            for (int row = 0; row < D; row++) m[col * 3 + row] = u.F[col * D + row];
        for (int col = 0; col < 3; col++) {
            for (int row = 0; row < 3; row++) r[col * 4 + row] = m[col * 3 + row];
            r[col * 4 + 3] = 0.f;
        }
        r[12] = u.x[0]; r[13] = u.x[1]; r[14] = D == 3 ? u.x[D - 1] : 0.f; r[15] = 0.f;
        const float base[4] = {r[16], r[17], r[18], r[19]};
        float col[4] = {base[0], base[1], base[2], base[3]};
        if (mode == WGS_RENDER_VELOCITY) {
            for (int k = 0; k < D; k++) col[k] = fabsf(u.v[k]) * dt * 100.0f + 0.2f;
        } else if (mode == WGS_RENDER_VOLUME) {
            Svd<D> sv;
            svd<D>(u.F, sv);
            float s[3] = {sv.s[0], sv.s[1], D == 3 ? sv.s[D - 1] : 0.f};
            // descending order, like the reference's SVD (wgebra Svd2/Svd3, third party)
            if (s[0] < s[1]) { float t = s[0]; s[0] = s[1]; s[1] = t; }
            if (D == 3) {
                if (s[1] < s[2]) { float t = s[1]; s[1] = s[2]; s[2] = t; }
                if (s[0] < s[1]) { float t = s[0]; s[0] = s[1]; s[1] = t; }
            }
            for (int k = 0; k < D; k++) col[k] = (1.0f - s[k]) / 0.005f + 0.2f;
        } else if (mode == WGS_RENDER_CDF_NORMALS) {
            bool zero = true;
            for (int k = 0; k < D; k++) zero = zero && u.nrm[k] == 0.f;
            col[0] = col[1] = col[2] = 0.f;
            if (!zero)
                for (int k = 0; k < D; k++) col[k] = (u.nrm[k] + 1.0f) / 2.0f;
        } else if (mode == WGS_RENDER_CDF_DISTANCES) {
            const float dd = u.dist / (h * 1.5f);
            col[0] = dd > 0.f ? 0.f : fabsf(dd);
            col[1] = dd > 0.f ? fabsf(dd) : 0.f;
            col[2] = 0.f;
        } else if (mode == WGS_RENDER_CDF_SIGNS) {
            const uint32_t a = (u.aff >> 16) & (u.aff & 0xffffu);
            col[0] = (u.aff != 0u && a != 0u) ? 1.f : 0.f;
            col[1] = (u.aff != 0u && a == 0u) ? 1.f : 0.f;
            col[2] = 0.f;
        }
        r[20] = col[0]; r[21] = col[1]; r[22] = col[2]; r[23] = col[3];
    }
}

__global__ void k_export_positions(Dev d, int side, float *out) {
    const float *in = d.buf[side];
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < d.n; j += gridDim.x * blockDim.x) {
        const uint32_t pid = ldpid<D>(in, d.npad, j);
        const float4 xm = ldq(in, d.npad, P::XM, j);
        out[(size_t)pid * D + 0] = xm.x;
        out[(size_t)pid * D + 1] = xm.y;
        if (D == 3) out[(size_t)pid * D + D - 1] = xm.z;
    }
}

__global__ void k_export_grid(Dev d, uint32_t nblocks, bool cpic, wgs_node_record *out) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT;
    const uint32_t total = nblocks * NPB;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const uint32_t b = d.active[t >> 6], ln = t & 63u;
        const uint32_t node = b * NPB + ln;
        int bc[3] = {0, 0, 0};
        unpack_key<D>(d.block_key[b], bc);
        int l[3] = {(int)(ln & (BW - 1)), (int)((ln >> BS) & (BW - 1)), D == 3 ? (int)(ln >> (2 * BS)) : 0};
        wgs_node_record r;
        for (int k = 0; k < D; k++) r.cell[k] = bc[k] * BW + l[k];
        float4 v = d.nodes[node];
        r.velocity[0] = v.x;
        r.velocity[1] = v.y;
        if (D == 3) { r.velocity[D - 1] = v.z; r.mass = v.w; } else { r.mass = v.z; }
        NodeCdf c = {0.f, 0u, NONE, 0u};
        if (cpic) c = d.node_cdf[node];
        r.cdf_distance = c.distance;
        r.cdf_affinities = c.affinities;
        r.cdf_closest_id = c.closest_id;
        out[t] = r;
    }
}

__global__ void k_export_blocks(Dev d, uint32_t nblocks, wgs_block_record *out) {
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < nblocks; a += gridDim.x * blockDim.x) {
        const uint32_t b = d.active[a];
        int bc[3] = {0, 0, 0};
        unpack_key<D>(d.block_key[b], bc);
        wgs_block_record r;
        for (int k = 0; k < D; k++) r.virtual_id[k] = bc[k];
        r.first_particle = d.block_start[b];
        r.num_particles = d.block_count[b];
        out[a] = r;
    }
}

}  // namespace
