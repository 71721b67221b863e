// kernels_walls.h — domain walls (wgs_set_domain_walls): axis-aligned half-spaces of grid NODES whose velocity is projected after
// the grid update and in front of the fused G2P. NEW: the reference builds every container from CPIC collider cuboids; this is the
// boundary condition on the grid that costs one short launch and no collider slot.
// One launch of its own (capi_walls.inc launch_grid_walls), only on data that has walls set; nothing else knows about it. The
// walls travel as the kernel's second argument: Dev does not grow.
#pragma once

namespace wgs {

// The 2 * D faces in the order of wgs_set_domain_walls (face 2k = low face of axis k, 2k + 1 = its high face), struct of arrays:
// 72 bytes in both dimensions (the 2D library leaves faces 4 and 5 at WGS_WALL_NONE).
struct WallSet {
    uint32_t type[6];
    float friction[6];
    int32_t plane[6];
};

// One face on the running value of a node inside it. `vn` = the component INTO the wall.
//   STICKY:   v = 0
//   SLIP:     v[k] = 0, then vt *= max(0, 1 - friction |vn| / |vt|)   (Coulomb friction in velocity form)
//   SEPARATE: SLIP where vn > 0, otherwise untouched
// friction == 0 and |vt| == 0 leave vt bit for bit.
template <int D> __device__ __forceinline__ void wall_face(float *v, int k, bool high, uint32_t type, float friction) {
    const float vn = high ? v[k] : -v[k];
    if (type == WGS_WALL_STICKY) {
#pragma unroll
        for (int j = 0; j < D; j++) v[j] = 0.f;
        return;
    }
    if (type == WGS_WALL_SEPARATE && !(vn > 0.f)) return;
    v[k] = 0.f;
    if (!(friction > 0.f)) return;
    float t2 = 0.f;
#pragma unroll
    for (int j = 0; j < D; j++)
        if (j != k) t2 += v[j] * v[j];
    const float vt = sqrtf(t2);
    if (!(vt > 0.f)) return;
    const float s = fmaxf(0.f, 1.f - friction * fabsf(vn) / vt);
#pragma unroll
    for (int j = 0; j < D; j++)
        if (j != k) v[j] *= s;
}

// One wave per active block and turn, lane = node (the indexing of k_grid_update / gu_waves). A block whose cell range reaches no
// face — nearly every block of a scene — is skipped on its key alone (wave-uniform). A lane of a reached block applies the faces
// its own cell is in, in array order on the running value, and writes a CHANGED value back to d.nodes and to every slab entry the
// grid update wrote it to: the fused G2P stages a block's velocity tile from d.slab, the readers use d.nodes. The walk over the
// source slabs is that of the tail of k_grid_update<D, 0>: each (source block, position) pair belongs to exactly one (block, node,
// region), so no two lanes of the launch write the same entry. Plain loads and stores: the producers (P2G with the grid-update
// waves, or k_grid_update) are earlier launches on the same stream, the consumers later ones.
template <int D> __global__ __launch_bounds__(256) void k_grid_walls(Dev d, WallSet w) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT, TW = Dim<D>::TW, TILE = Dim<D>::TILE, NN = Dim<D>::NNBR;
    const uint32_t B = min(d.counters[CTR_NBLOCKS], d.cap);
    const uint32_t nwaves = gridDim.x * 4u;
    const int lane = (int)(threadIdx.x & 63u);
    const int l[3] = {lane & (BW - 1), (lane >> BS) & (BW - 1), D == 3 ? (lane >> (2 * BS)) : 0};
    for (uint32_t a = blockIdx.x * 4u + (threadIdx.x >> 6); a < B; a += nwaves) {
        const uint32_t b = d.active[a];
        int bc[3] = {0, 0, 0};
        unpack_key<D>(d.block_key[b], bc);
        bool reached = false;   // (wave-uniform: the wave is one block)
#pragma unroll
        for (int k = 0; k < D; k++) {
            const int lo = bc[k] * BW;
            reached |= w.type[2 * k] != WGS_WALL_NONE && lo <= w.plane[2 * k];
            reached |= w.type[2 * k + 1] != WGS_WALL_NONE && lo + BW - 1 >= w.plane[2 * k + 1];
        }
        if (!reached) continue;
        const uint32_t node = b * NPB + (uint32_t)lane;
        const float4 old = d.nodes[node];
        float v[3] = {old.x, old.y, D == 3 ? old.z : 0.f};
#pragma unroll
        for (int f = 0; f < 2 * D; f++) {
            const int k = f >> 1, c = bc[k] * BW + l[k];
            const bool inside = (f & 1) ? c >= w.plane[f] : c <= w.plane[f];
            if (w.type[f] != WGS_WALL_NONE && inside) wall_face<D>(v, k, (f & 1) != 0, w.type[f], w.friction[f]);
        }
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
