// kernels_remove.h — particles removed at run time (include/wgsparkl_hip_remove.h): mark, scan, compact.
//   mark     k_remove_mark: one thread per slot of the current buffer decides the regions' membership from the stored position and writes
//            keep[id]; k_remove_keep_of_mask does the same from a caller's mask, which is by id already.
//   scan     keep (by id) -> new_index (exclusive count of the kept ids in front) and the total, as THREE launches: k_remove_tile_sums
//            (one sum per tile of REMOVE_TILE ids), k_remove_scan_tiles (ONE workgroup scans the tile sums in a loop),
//            k_remove_apply. No workgroup waits for another: the launches' order on the stream is the only dependency.
//   compact  k_remove_compact gathers a survivor — every quad of its slot, its cdf stamp, its model byte — from the current buffer into
//            slot new_index[id] of the OTHER buffer and writes its new id there; k_remove_settle copies [0, kept) back into the current
//            buffer and zeroes the vacated slots [kept, n_old) of both (what a reserved, never filled slot holds after creation).
//            k_remove_tables / k_remove_tables_back do the same for the by-id tables of the handle through a scratch copy.
// A raw copy of ALL quads is right in every layout (kernels_emit.h pack_particle lists them): XM.w of the uniform material, the fluid's
// collapsed F, the packed DP1 of uni_dp 2 travel with their quads, and since both buffers hold the compacted slots afterwards, the
// shared DP0 / DP2 of uni_dp 1 / 2 stand in both. Plain vector stores; every bound is a launch argument.
// Included last by capi.hip: no kernel that existed changes its place in the code object. The launches are in capi_remove.inc.
#pragma once

namespace {

constexpr uint32_t REMOVE_THREADS = 256;
constexpr uint32_t REMOVE_PER_THREAD = 4;
constexpr uint32_t REMOVE_TILE = REMOVE_THREADS * REMOVE_PER_THREAD;   // ids per tile of the scan

// The regions of one pass, a by-value kernel argument (scalar loads at fixed offsets, no scratch): the sinks that are due, in array order.
struct SinkSet {
    uint32_t n;
    wgs_sink s[WGS_MAX_SINKS];
};

// Membership of include/wgsparkl_hip_remove.h: every rounding a statement of its own (-ffp-contract=on fuses inside one expression only).
template <int DIM> __device__ __forceinline__ bool sink_takes(const wgs_sink &k, const float *x) {
    bool inside;
    if (k.region == (uint32_t)WGS_REGION_BOX) {
        inside = true;
#pragma unroll
        for (int c = 0; c < DIM; c++) {
            const float dc = x[c] - k.center[c];
            inside = inside && (fabsf(dc) <= k.half[c]);
        }
    } else {
        const float d0 = x[0] - k.center[0];
        const float d1 = x[1] - k.center[1];
        float s = d0 * d0;
        const float t1 = d1 * d1;
        s = s + t1;
        if constexpr (DIM == 3) {
            const float d2 = x[2] - k.center[2];
            const float t2 = d2 * d2;
            s = s + t2;
        }
        const float r2 = k.half[0] * k.half[0];
        inside = s <= r2;
    }
    return k.side == (uint32_t)WGS_SINK_OUTSIDE ? !inside : inside;
}

// keep[id] and the per-sink counts (counts[e], e < set.n: particles the e-th region of the set takes and none before it does).
// Whole waves run to the end (the wave sums use every lane); a lane behind the last slot takes part with nothing.
template <int DIM> __global__ __launch_bounds__(REMOVE_THREADS) void k_remove_mark(Dev d, int side, uint32_t n, SinkSet set, uint8_t *keep, uint32_t *counts) {
    const uint32_t j = blockIdx.x * REMOVE_THREADS + threadIdx.x;
    const bool live = j < n;
    uint32_t taker = WGS_MAX_SINKS;
    if (live) {
        const float *buf = d.buf[side];
        const float4 xm = ldq(buf, d.npad, Pl<DIM>::XM, j);
        const float x[3] = {xm.x, xm.y, xm.z};
#pragma unroll
        for (int e = WGS_MAX_SINKS - 1; e >= 0; e--)
            if ((uint32_t)e < set.n && sink_takes<DIM>(set.s[e], x)) taker = (uint32_t)e;
        const uint32_t pid = ldpid<DIM>(buf, d.npad, j);
        if (pid < n) keep[pid] = taker == (uint32_t)WGS_MAX_SINKS ? 1 : 0;   // (ids are dense below n on single-domain data; the bound guards keep[] all the same)
        else taker = WGS_MAX_SINKS;
    }
#pragma unroll
    for (int e = 0; e < WGS_MAX_SINKS; e++) {
        if ((uint32_t)e >= set.n) break;   // (uniform)
        const uint32_t total = wave_sum_u32(taker == (uint32_t)e ? 1u : 0u);
        if ((threadIdx.x & 63u) == 0u && total != 0u) atomicAdd(&counts[e], total);
    }
}

// a caller's mask (by id, nonzero = remove) -> keep, in place or not
template <int DIM> __global__ void k_remove_keep_of_mask(const uint8_t *remove, uint8_t *keep, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = remove[i] == 0 ? 1 : 0;
}

// the kept ids among the REMOVE_PER_THREAD consecutive ids of this thread, bit k = id first + k
__device__ __forceinline__ uint32_t keep_bits(const uint8_t *keep, uint32_t first, uint32_t n) {
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t k = 0; k < REMOVE_PER_THREAD; k++)
        if (first + k < n && keep[first + k] != 0) bits |= 1u << k;
    return bits;
}

// exclusive prefix of `mine` over the workgroup's REMOVE_THREADS threads, and the workgroup's total: wave scans, the four wave totals through LDS
__device__ __forceinline__ uint32_t group_scan_excl(uint32_t mine, uint32_t *wave_totals /* LDS, 4 */, uint32_t *total) {
    const uint32_t incl = wave_scan_incl_u32(mine), wave = threadIdx.x >> 6;
    __syncthreads();   // (the last round's readers are done with wave_totals)
    if ((threadIdx.x & 63u) == 63u) wave_totals[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (uint32_t w = 0; w < REMOVE_THREADS / 64u; w++) {
        const uint32_t t = wave_totals[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    *total = all;
    return before + incl - mine;
}

// tile_sums[b] = kept ids of tile b
template <int DIM> __global__ __launch_bounds__(REMOVE_THREADS) void k_remove_tile_sums(const uint8_t *keep, uint32_t n, uint32_t *tile_sums) {
    __shared__ uint32_t wave_totals[REMOVE_THREADS / 64];
    const uint32_t first = (blockIdx.x * REMOVE_THREADS + threadIdx.x) * REMOVE_PER_THREAD;
    uint32_t total;
    group_scan_excl((uint32_t)__popc(keep_bits(keep, first, n)), wave_totals, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// ONE workgroup: tile_sums -> their exclusive scan, in place, REMOVE_THREADS at a time with a running carry; *total = the sum of all
template <int DIM> __global__ __launch_bounds__(REMOVE_THREADS) void k_remove_scan_tiles(uint32_t *tile_sums, uint32_t ntiles, uint32_t *total) {
    __shared__ uint32_t wave_totals[REMOVE_THREADS / 64];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < ntiles; base += REMOVE_THREADS) {   // (uniform: every thread runs every round)
        const uint32_t i = base + threadIdx.x;
        const uint32_t mine = i < ntiles ? tile_sums[i] : 0u;
        uint32_t round_total;
        const uint32_t excl = group_scan_excl(mine, wave_totals, &round_total);
        if (i < ntiles) tile_sums[i] = carry + excl;
        carry += round_total;
    }
    if (threadIdx.x == 0) *total = carry;
}

// new_index[i] = kept ids in front of i, for every i < n (a removed id gets the index the next survivor gets)
template <int DIM> __global__ __launch_bounds__(REMOVE_THREADS) void k_remove_apply(const uint8_t *keep, uint32_t n, const uint32_t *tile_offsets, uint32_t *new_index) {
    __shared__ uint32_t wave_totals[REMOVE_THREADS / 64];
    const uint32_t first = (blockIdx.x * REMOVE_THREADS + threadIdx.x) * REMOVE_PER_THREAD;
    const uint32_t bits = keep_bits(keep, first, n);
    uint32_t total;
    uint32_t at = tile_offsets[blockIdx.x] + group_scan_excl((uint32_t)__popc(bits), wave_totals, &total);
#pragma unroll
    for (uint32_t k = 0; k < REMOVE_PER_THREAD; k++) {
        if (first + k < n) new_index[first + k] = at;
        at += (bits >> k) & 1u;
    }
}

// survivor at slot j of the current buffer -> slot new_index[id] of the other one, with its new id; n_old slots
template <int DIM> __global__ void k_remove_compact(Dev d, int side, uint32_t n_old, const uint8_t *keep, const uint32_t *new_index) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_old) return;
    const float *cur = d.buf[side];
    float *other = d.buf[side ^ 1];
    const uint32_t pid = ldpid<DIM>(cur, d.npad, j);
    if (pid >= n_old || keep[pid] == 0) return;   // (ids are dense below n_old on single-domain data; the bound guards the tables all the same)
    const uint32_t q = new_index[pid];
#pragma unroll
    for (int quad = 0; quad < Pl<DIM>::NQ; quad++) stq(other, d.npad, quad, q, ldq(cur, d.npad, quad, j));
    stpid<DIM>(other, d.npad, q, q);
    ststamp<DIM>(other, d.npad, q, ldstamp<DIM>(cur, d.npad, j));   // (copied: the survivor's cdf is as old as it was)
    if (d.pmodel[0]) stmodel(d.pmodel[side ^ 1], q, ldmodel(d.pmodel[side], j));
}

// slots [0, kept) of the other buffer -> the current one; slots [kept, n_old) of both -> zero, the reserved slots' content
template <int DIM> __global__ void k_remove_settle(Dev d, int side, uint32_t n_old, uint32_t kept) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_old) return;
    float *cur = d.buf[side], *other = d.buf[side ^ 1];
    if (i < kept) {
#pragma unroll
        for (int quad = 0; quad < Pl<DIM>::NQ; quad++) stq(cur, d.npad, quad, i, ldq(other, d.npad, quad, i));
        stpid<DIM>(cur, d.npad, i, i);
        ststamp<DIM>(cur, d.npad, i, ldstamp<DIM>(other, d.npad, i));
        if (d.pmodel[0]) stmodel(d.pmodel[side], i, ldmodel(d.pmodel[side ^ 1], i));
    } else {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int quad = 0; quad < Pl<DIM>::NQ; quad++) {
            stq(cur, d.npad, quad, i, zero);
            stq(other, d.npad, quad, i, zero);
        }
        stpid<DIM>(cur, d.npad, i, 0u);
        stpid<DIM>(other, d.npad, i, 0u);
        ststamp<DIM>(cur, d.npad, i, 0u);
        ststamp<DIM>(other, d.npad, i, 0u);
        if (d.pmodel[0]) {
            stmodel(d.pmodel[0], i, 0u);
            stmodel(d.pmodel[1], i, 0u);
        }
    }
}

// The by-id tables of the handle (wgs_data::static_*) and their scratch copy: radius, dp (6), phase (2), flags — 10 words per id.
struct IdTables {
    float *radius, *dp, *phase;
    uint32_t *flags;
};

// survivor id p -> entry new_index[p] of the scratch tables; kept_from[new_index[p]] = p
template <int DIM> __global__ void k_remove_tables(IdTables from, IdTables to, uint32_t n_old, const uint8_t *keep, const uint32_t *new_index, uint32_t *kept_from) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_old || keep[p] == 0) return;
    const uint32_t q = new_index[p];
    to.radius[q] = from.radius[p];
#pragma unroll
    for (int k = 0; k < 6; k++) to.dp[(size_t)q * 6 + k] = from.dp[(size_t)p * 6 + k];
    to.phase[(size_t)q * 2] = from.phase[(size_t)p * 2];
    to.phase[(size_t)q * 2 + 1] = from.phase[(size_t)p * 2 + 1];
    to.flags[q] = from.flags[p];
    kept_from[q] = p;
}

// the scratch tables' [0, kept) -> the handle's; [kept, n_old) of the handle's -> zero
template <int DIM> __global__ void k_remove_tables_back(IdTables from, IdTables to, uint32_t n_old, uint32_t kept) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_old) return;
    const bool live = i < kept;
    to.radius[i] = live ? from.radius[i] : 0.f;
#pragma unroll
    for (int k = 0; k < 6; k++) to.dp[(size_t)i * 6 + k] = live ? from.dp[(size_t)i * 6 + k] : 0.f;
    to.phase[(size_t)i * 2] = live ? from.phase[(size_t)i * 2] : 0.f;
    to.phase[(size_t)i * 2 + 1] = live ? from.phase[(size_t)i * 2 + 1] : 0.f;
    to.flags[i] = live ? from.flags[i] : 0u;
}

}  // namespace
