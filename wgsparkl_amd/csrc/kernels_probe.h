// kernels_probe.h — device code of the Eulerian field output (include/wgsparkl_hip.h "Eulerian field output"): the grid of
// the last substep sampled at arbitrary points with the step's own stencil, and a dense window of its raw nodes. Read-only:
// nothing here writes simulation state, and Dev is what every other kernel gets. Kernels only; the entry points that launch
// them are in capi_probe.inc. The three kernels are templates on the dimension for one reason: a kernel template is emitted where a
// host function first launches it — capi_probe.inc, the last part of capi.hip —, so they land behind every kernel that existed and none
// of those changes its place in the code object (a plain kernel would be emitted in front of the step's templates).
//
// "The grid" is what k_export_grid (kernels_readback.h) walks: the blocks on the active list, [0, min(CTR_NBLOCKS, cap)).
// A block's epoch stamp does NOT say that — the fused G2P of a substep already stamps the blocks of the next one
// (Dev::bin_next) — so the sampler, which finds blocks through the table, tests membership of that very list: k_probe_mark
// writes the call's ticket into a scratch word per listed block id, and a block counts where its word holds the ticket.
#pragma once

namespace {

constexpr int PROBE_WORDS = D + DD + 2;   // words of a wgs_grid_sample: velocity, velocity_gradient, density, active_nodes
constexpr int PROBE_THREADS = 256;
constexpr float PROBE_MAX_CELLS = 4194304.0f;   // 2^22: beyond every cell of the key range (2D: 2^18, 3D: 2^12), far inside int

// index into the 2^D blocks of a stencil; the 3D branch below is parsed (never run) in the 2D library too
[[maybe_unused]] constexpr int k8(int k) { return D == 3 ? k : 0; }

// mark[id] = ticket for the ids on the active list of the last substep (tickets only grow: no clearing between calls)
template <int DIM> __global__ void k_probe_mark(Dev d, uint32_t *mark, uint32_t ticket) {
    const uint32_t nblocks = min(d.counters[CTR_NBLOCKS], d.cap);
    for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < nblocks; a += gridDim.x * blockDim.x) {
        const uint32_t id = d.active[a];
        if (id < d.cap) mark[id] = ticket;
    }
}

// The physical ids of the 2^D blocks a stencil can reach (NONE: not wanted, not in the table, or not on the active list),
// probing in lockstep like hmap_find_many (device_math.h): the loads of all unresolved keys of a round are issued together.
// Every lane of the wave must call it. Bounded: at most hmask + 1 rounds, ids checked against the capacity.
__device__ inline void probe_find_blocks(const Dev &d, const uint32_t *mark, uint32_t ticket, const uint32_t *keys, const bool *wanted, uint32_t *out) {
    constexpr int K = 1 << D;
    uint32_t slot[K], id[K];
    bool pend[K], hit[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        slot[k] = hash_key(keys[k]) & d.hmask;
        pend[k] = wanted[k];
        hit[k] = false;
    }
    for (uint32_t probe = 0; probe <= d.hmask; ++probe) {
        uint32_t st[K];
#pragma unroll
        for (int k = 0; k < K; k++) st[k] = pend[k] ? d.hkeys[slot[k]] : NONE;
        bool more = false;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (!pend[k]) continue;
            if (st[k] == keys[k]) { hit[k] = true; pend[k] = false; }
            else if (st[k] == NONE) pend[k] = false;
            else { slot[k] = (slot[k] + 1u) & d.hmask; more = true; }
        }
        if (__ballot(more) == 0ull) break;
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        id[k] = hit[k] ? d.hvals[slot[k]] : NONE;
        if (id[k] >= d.cap) id[k] = NONE;
    }
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = (id[k] != NONE && mark[id[k]] == ticket) ? id[k] : NONE;
}

// One sample: what G2P gives a particle at x before the speed cap, plus the density sum w m / h^D and the number of
// stencil nodes in active blocks. Summation order: the TENSOR-PRODUCT order of g2p_body.inc's plain body (x, then y, then
// z), expression for expression, with the node mass carried as one more component; one thread, one fixed order.
__device__ inline void probe_sample(const Dev &d, const uint32_t *mark, uint32_t ticket, uint32_t nblocks, const float *xin, bool lane_on, float *rec) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT, K = 1 << D;
    const float h = d.h, inv_h = d.inv_h;
    const float invd = 4.0f / (h * h);
    // ---- bad points are decided on the floats, before any conversion
    bool ok = lane_on && nblocks != 0u;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) {
        ok = ok && (xin[k] - xin[k] == 0.f) && (fabsf(xin[k]) * inv_h < PROBE_MAX_CELLS);
    }
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = ok ? xin[k] : 0.f;
    int cell[D], b0[D], b1[D];
#pragma unroll
    for (int k = 0; k < D; k++) {
        cell[k] = assoc_cell(x[k], h, inv_h, d.h_pow2 != 0u);
        b0[k] = cell[k] >> BS;
        b1[k] = (cell[k] + 2) >> BS;   // BW >= 3: the stencil's three cells span at most two blocks per axis
    }
    uint32_t keys[K];
    bool wanted[K];
#pragma unroll
    for (int o = 0; o < K; o++) {
        int bc[3] = {0, 0, 0};
        bool distinct = true;
#pragma unroll
        for (int k = 0; k < D; k++) {
            bc[k] = ((o >> k) & 1) ? b1[k] : b0[k];
            distinct = distinct && (!((o >> k) & 1) || b1[k] != b0[k]);
        }
        ok = ok && block_in_key_range<D>(bc);
        keys[o] = pack_key<D>(bc);
        wanted[o] = distinct;
    }
#pragma unroll
    for (int o = 0; o < K; o++) wanted[o] = wanted[o] && ok;
    uint32_t ids[K];
    probe_find_blocks(d, mark, ticket, keys, wanted, ids);

    float ref[D], w[D][3];
    bool hi[D][3];     // stencil cell s of axis k lies in the upper block
    uint32_t loc[D][3];  // its coordinate inside its block
#pragma unroll
    for (int k = 0; k < D; k++) {
        ref[k] = (float)cell[k] * h - x[k];
        eval_all(-ref[k] * inv_h, w[k]);
#pragma unroll
        for (int s = 0; s < 3; s++) {
            hi[k][s] = ((cell[k] + s) >> BS) != b0[k];
            loc[k][s] = (uint32_t)((cell[k] + s) & (BW - 1));
        }
    }
    constexpr int NC = D + 1;   // velocity components + mass
    constexpr int SZN = D == 3 ? 3 : 1;
    float acc[NC], G[D][D];   // acc: v, sum w m; G[c][r] = sum_n w_n s_c(n) v_n,r
    uint32_t nactive = 0u;
#pragma unroll
    for (int k = 0; k < NC; k++) acc[k] = 0.f;
#pragma unroll
    for (int c = 0; c < D; c++)
#pragma unroll
        for (int r = 0; r < D; r++) G[c][r] = 0.f;
    const float wx1 = w[0][1], wx2 = 2.0f * w[0][2];
#pragma unroll
    for (int sz = 0; sz < SZN; sz++) {
        float Pz[NC], Gxz[D], Gyz[D];
#pragma unroll
        for (int k = 0; k < NC; k++) Pz[k] = 0.f;
#pragma unroll
        for (int k = 0; k < D; k++) { Gxz[k] = 0.f; Gyz[k] = 0.f; }
        const bool hz = D == 3 ? hi[D - 1][sz] : false;
        const uint32_t lz = D == 3 ? loc[D - 1][sz] << (2 * BS) : 0u;
#pragma unroll
        for (int sy = 0; sy < 3; sy++) {
            // the two blocks of this row of the stencil (selects on static elements: no array indexed at run time)
            const bool hy = hi[1][sy];
            uint32_t id_lo, id_hi;
            if constexpr (D == 3) {
                id_lo = hz ? (hy ? ids[k8(6)] : ids[k8(4)]) : (hy ? ids[2] : ids[0]);
                id_hi = hz ? (hy ? ids[k8(7)] : ids[k8(5)]) : (hy ? ids[3] : ids[1]);
            } else {
                id_lo = hy ? ids[2] : ids[0];
                id_hi = hy ? ids[3] : ids[1];
            }
            // (hi on an axis whose two blocks coincide never happens: hi compares with b0)
            const uint32_t row = (loc[1][sy] << BS) + lz;
            float4 nd[3];
#pragma unroll
            for (int sx = 0; sx < 3; sx++) {
                const uint32_t id = hi[0][sx] ? id_hi : id_lo;
                nd[sx] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id != NONE) {
                    nd[sx] = d.nodes[(size_t)id * NPB + row + loc[0][sx]];
                    nactive++;
                }
            }
            float a0[NC], a1[NC], a2[NC];
            a0[0] = nd[0].x; a0[1] = nd[0].y; a1[0] = nd[1].x; a1[1] = nd[1].y; a2[0] = nd[2].x; a2[1] = nd[2].y;
            if constexpr (D == 3) {
                a0[2] = nd[0].z; a1[2] = nd[1].z; a2[2] = nd[2].z;
                a0[NC - 1] = nd[0].w; a1[NC - 1] = nd[1].w; a2[NC - 1] = nd[2].w;
            } else {
                a0[NC - 1] = nd[0].z; a1[NC - 1] = nd[1].z; a2[NC - 1] = nd[2].z;
            }
            const float wy = w[1][sy];
#pragma unroll
            for (int k = 0; k < NC; k++) {
                const float p = w[0][0] * a0[k] + w[0][1] * a1[k] + w[0][2] * a2[k];
                Pz[k] += wy * p;
                if (k < D) {
                    const float gx = wx1 * a1[k] + wx2 * a2[k];
                    Gxz[k] += wy * gx;
                    if (sy > 0) Gyz[k] += ((float)sy * wy) * p;
                }
            }
        }
        float wz = 1.f;
        if constexpr (D == 3) wz = w[D - 1][sz];
#pragma unroll
        for (int k = 0; k < NC; k++) acc[k] += wz * Pz[k];
#pragma unroll
        for (int k = 0; k < D; k++) {
            G[0][k] += wz * Gxz[k];
            G[1][k] += wz * Gyz[k];
            if constexpr (D == 3) G[D - 1][k] += ((float)sz * wz) * Pz[k];
        }
    }
    float cell_volume = h * h;
    if constexpr (D == 3) cell_volume *= h;
    // a bad point (and everything while no block is active) is an all-zero record, +0 in every word
#pragma unroll
    for (int k = 0; k < D; k++) rec[k] = ok ? acc[k] : 0.f;
#pragma unroll
    for (int c = 0; c < D; c++)
#pragma unroll
        for (int r = 0; r < D; r++) rec[D + c * D + r] = ok ? invd * (acc[r] * ref[c] + h * G[c][r]) : 0.f;
    rec[D + DD] = ok ? acc[NC - 1] / cell_volume : 0.f;
    rec[D + DD + 1] = __uint_as_float(ok ? nactive : 0u);
}

// One sample per lane, blocks of PROBE_THREADS samples in a grid-stride loop. A workgroup's records are contiguous in
// `out`, so they go through LDS and leave as whole rows of consecutive words (a lane storing its own 56-byte record would
// touch 28 cache lines per store instruction). No atomics; what a record holds depends on its point and the grid only.
template <int DIM> __global__ __launch_bounds__(PROBE_THREADS) void k_probe_sample(Dev d, const uint32_t *mark, uint32_t ticket, const float *points, uint32_t n, float *out) {
    __shared__ float s_rec[PROBE_THREADS * PROBE_WORDS];
    const uint32_t nblocks = min(d.counters[CTR_NBLOCKS], d.cap);
    for (uint32_t base = blockIdx.x * PROBE_THREADS; base < n; base += gridDim.x * PROBE_THREADS) {   // (uniform over the workgroup)
        const uint32_t i = base + threadIdx.x;
        const bool lane_on = i < n;
        float x[D];
#pragma unroll
        for (int k = 0; k < D; k++) x[k] = lane_on ? points[(size_t)i * D + k] : 0.f;
        float rec[PROBE_WORDS];
        probe_sample(d, mark, ticket, nblocks, x, lane_on, rec);
#pragma unroll
        for (int k = 0; k < PROBE_WORDS; k++) s_rec[threadIdx.x * PROBE_WORDS + k] = rec[k];
        __syncthreads();
        const uint32_t words = min((uint32_t)PROBE_THREADS, n - base) * PROBE_WORDS;
        float *dst = out + (size_t)base * PROBE_WORDS;
        for (uint32_t t = threadIdx.x; t < words; t += PROBE_THREADS) dst[t] = s_rec[t];
        __syncthreads();
    }
}

struct ProbeWindow { int lo[3]; uint32_t dims[3]; };

// The raw nodes of the active list scattered into a dense window (cleared by the caller): node (i, j[, k]) of the window
// is world cell lo + (i, j[, k]) at index i + dims[0] * (j + dims[1] * k), D + 1 floats each: velocity, mass.
template <int DIM> __global__ void k_probe_window(Dev d, ProbeWindow win, float *out) {
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT;
    const uint32_t total = min(d.counters[CTR_NBLOCKS], d.cap) * NPB;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const uint32_t b = d.active[t >> 6], ln = t & 63u;
        if (b >= d.cap) continue;
        int bc[3] = {0, 0, 0};
        unpack_key<D>(d.block_key[b], bc);
        const int l[3] = {(int)(ln & (BW - 1)), (int)((ln >> BS) & (BW - 1)), D == 3 ? (int)(ln >> (2 * BS)) : 0};
        bool inside = true;
        size_t idx = 0, stride = 1;
#pragma unroll
        for (int k = 0; k < D; k++) {
            const long long rel = (long long)(bc[k] * BW + l[k]) - (long long)win.lo[k];
            inside = inside && rel >= 0 && rel < (long long)win.dims[k];
            idx += (size_t)rel * stride;
            stride *= win.dims[k];
        }
        if (!inside) continue;
        const float4 v = d.nodes[(size_t)b * NPB + ln];
        float *r = out + idx * (D + 1);
        r[0] = v.x;
        r[1] = v.y;
        r[2] = v.z;   // (2D: the mass)
        if (D == 3) r[D] = v.w;
    }
}

}  // namespace
