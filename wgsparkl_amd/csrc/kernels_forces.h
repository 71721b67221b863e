// kernels_forces.h — force fields (wgs_set_force_fields, include/wgsparkl_hip_forces.h): uniform, radial, vortex and drag rules on the
// grid NODES' velocities, each inside a region (everywhere, a box, a ball), applied behind the grid update and in front of the domain
// walls and the fused G2P. NEW: the reference's only body force is the one gravity vector of its SimulationParams.
// One launch of its own (capi_forces.inc launch_grid_forces), only on data that has a field set; nothing else knows about it. The
// fields travel as the kernel's second argument: Dev does not grow.
#pragma once

namespace wgs {

// The fields in the order of wgs_set_force_fields, struct of arrays: 548 bytes in both dimensions. `n` = entries in use (the rest is
// zero: WGS_FORCE_NONE). `vec` of a 3D VORTEX holds the axis normalised by the host (in double, rounded once); `softening` its square
// root as the caller gave it.
struct ForceSet {
    uint32_t n;
    uint32_t kind[WGS_MAX_FORCE_FIELDS], falloff[WGS_MAX_FORCE_FIELDS], region[WGS_MAX_FORCE_FIELDS];
    float strength[WGS_MAX_FORCE_FIELDS], softening[WGS_MAX_FORCE_FIELDS];
    float center[WGS_MAX_FORCE_FIELDS][3], vec[WGS_MAX_FORCE_FIELDS][3], rcenter[WGS_MAX_FORCE_FIELDS][3], rhalf[WGS_MAX_FORCE_FIELDS][3];
};

// w_p(q): 1, 1/sqrt(q), 1/q, 1/(q sqrt(q)) — a correctly rounded root and correctly rounded quotients (the truth's bound counts them)
__device__ __forceinline__ float force_falloff(uint32_t p, float q) {
    if (p == 0u) return 1.0f;
    if (p == 2u) return 1.0f / q;
    const float rs = 1.0f / sqrtf(q);
    return p == 1u ? rs : rs / q;
}

// Does the region of field i reach the interval [xlo, xhi] of node positions on every axis? fl(x - c) does not decrease with x, so
// fl(xhi - c) < -half puts every node of the interval below the region's bounding box, fl(xlo - c) > half above it: exactly the per-axis
// test force_inside makes, on the interval's ends. A ball is culled by its bounding box.
template <int D> __device__ __forceinline__ bool force_reaches(const ForceSet &w, uint32_t i, const float *xlo, const float *xhi) {
    if (w.region[i] == WGS_REGION_ALL) return true;
    bool reached = true;
#pragma unroll
    for (int k = 0; k < D; k++) {
        const float half = w.region[i] == WGS_REGION_BALL ? w.rhalf[i][0] : w.rhalf[i][k];
        const float lo = xlo[k] - w.rcenter[i][k], hi = xhi[k] - w.rcenter[i][k];
        reached &= !(hi < -half || lo > half);
    }
    return reached;
}

// Is the node at x inside the region of field i? BOX: |x_k - c_k| <= half_k on every axis. BALL: inside its bounding box (implied in
// exact arithmetic; in fp32 it makes the cull above exact) and |x - c|^2 <= half_0^2.
template <int D> __device__ __forceinline__ bool force_inside(const ForceSet &w, uint32_t i, const float *x) {
    if (w.region[i] == WGS_REGION_ALL) return true;
    const bool ball = w.region[i] == WGS_REGION_BALL;
    bool in = true;
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < D; k++) {
        const float half = ball ? w.rhalf[i][0] : w.rhalf[i][k];
        const float dx = x[k] - w.rcenter[i][k];
        in &= fabsf(dx) <= half;
        d2 += dx * dx;
    }
    if (ball) in &= d2 <= w.rhalf[i][0] * w.rhalf[i][0];
    return in;
}

// Field i on the running value v of the node at x (the rule of include/wgsparkl_hip_forces.h). kind, falloff and region are scalars:
// the branches are wave-uniform.
template <int D> __device__ __forceinline__ void force_apply(const ForceSet &w, uint32_t i, const float *x, float dt, float *v) {
    const uint32_t kind = w.kind[i];
    if (kind == WGS_FORCE_UNIFORM) {
#pragma unroll
        for (int k = 0; k < D; k++) v[k] += dt * w.vec[i][k];
    } else if (kind == WGS_FORCE_DRAG) {
        const float kdt = fminf(w.strength[i] * dt, 1e30f);
        const float s = kdt / (1.0f + kdt);
        const float keep = 1.0f - s;   // (v + s (vec - v) as (1 - s) v + s vec: s == 1 leaves vec bit for bit)
#pragma unroll
        for (int k = 0; k < D; k++) v[k] = keep * v[k] + s * w.vec[i][k];
    } else if (kind == WGS_FORCE_RADIAL) {
        float r[3] = {0.f, 0.f, 0.f};
        float q = w.softening[i] * w.softening[i];
#pragma unroll
        for (int k = 0; k < D; k++) {
            r[k] = w.center[i][k] - x[k];
            q += r[k] * r[k];
        }
        const float c = dt * w.strength[i] * force_falloff(w.falloff[i], q);
#pragma unroll
        for (int k = 0; k < D; k++) v[k] += c * r[k];
    } else if (kind == WGS_FORCE_VORTEX) {
        float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; k++) r[k] = x[k] - w.center[i][k];
        float t[3] = {0.f, 0.f, 0.f};   // n x rp
        float q = w.softening[i] * w.softening[i];
        if constexpr (D == 2) {
            q += r[0] * r[0] + r[1] * r[1];
            t[0] = -r[1];
            t[1] = r[0];
        } else {
            const float n[3] = {w.vec[i][0], w.vec[i][1], w.vec[i][2]};
            const float rn = r[0] * n[0] + r[1] * n[1] + r[2] * n[2];
            const float rp[3] = {r[0] - rn * n[0], r[1] - rn * n[1], r[2] - rn * n[2]};
            q += rp[0] * rp[0] + rp[1] * rp[1] + rp[2] * rp[2];
            t[0] = n[1] * rp[2] - n[2] * rp[1];
            t[1] = n[2] * rp[0] - n[0] * rp[2];
            t[2] = n[0] * rp[1] - n[1] * rp[0];
        }
        const float c = dt * w.strength[i] * force_falloff(w.falloff[i], q);
#pragma unroll
        for (int k = 0; k < D; k++) v[k] += c * t[k];
    }
}

// One wave per active block and turn, lane = node (the indexing of k_grid_walls). A block whose node box misses the bounding box of
// every region of every field is skipped on its key alone (wave-uniform). A lane of a reached block whose node has mass applies the
// fields whose region holds its node, in array order on the running value, and writes a CHANGED velocity back to d.nodes and to every
// slab entry the grid update wrote it to (the walk of k_grid_walls: each (source block, position) pair belongs to exactly one (block,
// node, region), so no two lanes of the launch write the same entry). Plain loads and stores, no LDS, no atomics: the producers (P2G
// with the grid-update waves, or k_grid_update) are earlier launches on the same stream, the consumers (k_grid_walls, the fused G2P,
// the readers) later ones.
template <int D> __global__ __launch_bounds__(256) void k_grid_forces(Dev d, ForceSet w) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT, TW = Dim<D>::TW, TILE = Dim<D>::TILE, NN = Dim<D>::NNBR;
    const uint32_t B = min(d.counters[CTR_NBLOCKS], d.cap);
    const uint32_t nwaves = gridDim.x * 4u;
    const uint32_t nf = min(w.n, (uint32_t)WGS_MAX_FORCE_FIELDS);
    const float dt = d.sp->dt;
    const float h = d.h;
    const int lane = (int)(threadIdx.x & 63u);
    const int l[3] = {lane & (BW - 1), (lane >> BS) & (BW - 1), D == 3 ? (lane >> (2 * BS)) : 0};
    for (uint32_t a = blockIdx.x * 4u + (threadIdx.x >> 6); a < B; a += nwaves) {
        const uint32_t b = d.active[a];
        int bc[3] = {0, 0, 0};
        unpack_key<D>(d.block_key[b], bc);
        float xlo[3] = {0.f, 0.f, 0.f}, xhi[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; k++) {
            xlo[k] = (float)(bc[k] * BW) * h;
            xhi[k] = (float)(bc[k] * BW + BW - 1) * h;
        }
        bool reached = false;   // (wave-uniform: the wave is one block)
        for (uint32_t i = 0; i < nf; i++)
            if (w.kind[i] != WGS_FORCE_NONE) reached |= force_reaches<D>(w, i, xlo, xhi);
        if (!reached) continue;
        const uint32_t node = b * NPB + (uint32_t)lane;
        const float4 old = d.nodes[node];
        if (!((D == 3 ? old.w : old.z) > 0.f)) continue;   // (a massless node is never touched)
        float x[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; k++) x[k] = (float)(bc[k] * BW + l[k]) * h;
        float v[3] = {old.x, old.y, D == 3 ? old.z : 0.f};
        for (uint32_t i = 0; i < nf; i++)
            if (w.kind[i] != WGS_FORCE_NONE && force_inside<D>(w, i, x)) force_apply<D>(w, i, x, dt, v);
        bool changed = __float_as_uint(v[0]) != __float_as_uint(old.x) || __float_as_uint(v[1]) != __float_as_uint(old.y);
        if (D == 3) changed |= __float_as_uint(v[2]) != __float_as_uint(old.z);
        if (!changed) continue;
        const float4 nv = D == 3 ? make_float4(v[0], v[1], v[2], old.w) : make_float4(v[0], v[1], old.z, old.w);   // (mass untouched)
#pragma unroll
        for (int o = 0; o < NN; o++) {
            const int tt[3] = {l[0] + BW * (o & 1), l[1] + BW * ((o >> 1) & 1), l[2] + BW * ((o >> 2) & 1)};
            const bool in_tile = tt[0] < TW && tt[1] < TW && (D == 2 || tt[2] < TW);
            if (!in_tile) continue;
            const uint32_t src = d.act_src[a * 8u + (uint32_t)o];   // (k_regroup: "-" neighbour with particles, else NONE)
            if (src == NONE) continue;
            d.slab[(size_t)src * TILE + slab_pos<D>(o, l)] = nv;
        }
        d.nodes[node] = nv;
    }
}

}  // namespace wgs
