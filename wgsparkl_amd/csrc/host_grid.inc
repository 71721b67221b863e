// host_grid.inc — the arrays sized by the block capacity and the host's care for them: alloc_grid (the ONE list of those
// arrays), enable_impulses, clear_table, grow_grid, and the host's looks at the device counters that decide about growth and table
// rebuilds (maintain_grid on the pinned watch, fetch_counters at a synchronisation), with sticky_status and resolve_timings
// as the other two things a synchronising caller asks for. Host code only: nothing here launches a kernel.

namespace {

// Every array sized by the block capacity (dev.cap, dev.hmask set by the caller) — the grid group of DeviceMemory. All of
// them are rebuilt by the sort of a table-rebuild substep, so a fresh zeroed set is a valid state (see grow_grid).
// An array is listed HERE AND NOWHERE ELSE: the optional ones under the flag that says the data uses them, and whoever
// sets such a flag later (enable_impulses, wgs_set_rigid_particles) calls this with `missing_only` to get what it adds.
wgs_status alloc_grid(wgs_data *d, bool missing_only = false) {
    Dev &dev = d->dev;
    const size_t hcap = (size_t)dev.hmask + 1, cap = dev.cap, nchunk = (cap + SCAN_CHUNK - 1) / SCAN_CHUNK;
    auto grid_array = [&](auto **ptr, size_t count) {
        return missing_only && *ptr ? WGS_OK : dev_alloc(d, ptr, count, MemGroup::grid);
    };
    WGS_TRY(grid_array(&dev.hkeys, hcap));
    WGS_TRY(grid_array(&dev.hvals, hcap));
    WGS_TRY(grid_array(&dev.block_key, cap));
    if (!(dev.dbg & DBG_NO_EVICTION)) {   // (eviction of blocks long inactive — slabs of a decomposition too since round 6)
        WGS_TRY(grid_array(&dev.block_slot, cap));
        WGS_TRY(grid_array(&dev.free_ids, cap));
    }
    WGS_TRY(grid_array(&dev.block_count, cap));
    WGS_TRY(grid_array(&dev.block_stamp, cap));
    WGS_TRY(grid_array(&dev.links_epoch, cap));
    WGS_TRY(grid_array(&dev.block_acc, cap));
    WGS_TRY(grid_array(&dev.block_dirty, cap));
    WGS_TRY(grid_array(&dev.blk_narr, cap));
    WGS_TRY(grid_array(&dev.block_ident, cap));
    WGS_TRY(grid_array(&dev.blk_arr, cap * BLK_ARR));
    WGS_TRY(grid_array(&dev.active, cap));
    WGS_TRY(grid_array(&dev.block_start, cap));
    WGS_TRY(grid_array(&dev.act_info, cap));
    WGS_TRY(grid_array(&dev.act_cells, cap * NPB));
    WGS_TRY(grid_array(&dev.nbr_plus, cap * 8));
    WGS_TRY(grid_array(&dev.nbr_minus, cap * 8));
    WGS_TRY(grid_array(&dev.nbr_known, cap * 16));
    WGS_TRY(grid_array(&dev.act_src, cap * 8));
    WGS_TRY(grid_array(&dev.cell_head, cap * NPB));
    WGS_TRY(grid_array(&dev.chunk_a, nchunk));
    WGS_TRY(grid_array(&dev.chunk_b, nchunk));
    WGS_TRY(grid_array(&dev.group_a, nchunk * SORT_THREADS));
    WGS_TRY(grid_array(&dev.group_b, nchunk * SORT_THREADS));
    WGS_TRY(grid_array(&dev.cell_start, cap * NPB));
    WGS_TRY(grid_array(&dev.cell_cursor, cap * NPB));
    WGS_TRY(grid_array(&dev.nodes, cap * NPB));
    WGS_TRY(grid_array(&dev.node_cdf, cap * NPB));
    WGS_TRY(grid_array(&dev.slab, cap * Dim<D>::TILE));
    WGS_TRY(grid_array(&dev.slab_epoch, cap));
    WGS_TRY(grid_array(&dev.block_cdf_gen, cap));
    WGS_TRY(grid_array(&dev.block_cpic, cap));
    WGS_TRY(grid_array(&dev.block_cdf_summ, cap));
    WGS_TRY(grid_array(&dev.pcdf_done, cap));
    WGS_TRY(grid_array(&dev.cpic_list, cap * 8));
    dev.visit_cap = dev.npad / 512u + 2u * dev.cap + 16u;
    WGS_TRY(grid_array(&dev.visit_list, (size_t)dev.visit_cap * 8));
    if (dev.sharded) WGS_TRY(grid_array(&dev.halo_list, cap * HALO_ENT));
    if (d->two_way) WGS_TRY(grid_array(&dev.imp_slab, cap * Dim<D>::TILE * (D == 3 ? 2 : 1)));   // per-block partial node impulses
    if (d->mesh_cdf) {
        WGS_TRY(grid_array(&dev.mesh_min, cap * NPB));
        WGS_TRY(grid_array(&dev.mesh_aff, cap * NPB));
    }
    return WGS_OK;
}

// Bodies that move need the impulse accumulation of P2G (rigid_impulses.wgsl reads it every substep). On sharded data
// every rank accumulates the impulses of its own particles and the fixed-point sums are reduced over the ranks before
// integrate_bodies (wgs_sharded_step: ncclAllReduce of 16 x 8 int32; integers, so the order does not matter).
wgs_status enable_impulses(wgs_data *d) {
    if (d->two_way) return WGS_OK;
    d->two_way = true;
    const wgs_status st = alloc_grid(d, true);   // (imp_slab)
    if (st != WGS_OK) d->two_way = false;
    return st;
}

// Every slot of the table of block ids empty, on the data's stream; `ids_too`: and the ids handed out anew (reset_hmap, device_math.h).
wgs_status clear_table(wgs_data *d, bool ids_too) {
    const Dev &dev = d->dev;
    HIP_TRY(hipMemsetAsync(dev.hkeys, 0xff, sizeof(uint32_t) * ((size_t)dev.hmask + 1), d->stream));
    HIP_TRY(hipMemsetAsync(dev.hvals, 0xff, sizeof(uint32_t) * ((size_t)dev.hmask + 1), d->stream));
    if (!ids_too) return WGS_OK;
    HIP_TRY(hipMemsetAsync(dev.counters + CTR_NPHYS, 0, sizeof(uint32_t), d->stream));
    HIP_TRY(hipMemsetAsync(dev.counters + CTR_NFREE, 0, 3 * sizeof(uint32_t), d->stream));   // (free list, insertion count, marks: layout.h)
    return WGS_OK;
}

// SURVEY 8f4, second half — the reference's resize loop is a stub (src/grid/grid.rs:43-45,116-117: "TODO: resize the
// hashmap and retry"). Here the block capacity doubles BEFORE the table fills: a new zeroed set of grid arrays replaces
// the old one and the next substep rebuilds the table from the particles (the same full pass a table rebuild runs).
// Particle state is untouched, so nothing is lost; the stream is drained once (rare).
wgs_status grow_grid(wgs_data *d, uint32_t new_cap) {
    Dev &dev = d->dev;
    HIP_TRY(hipStreamSynchronize(d->stream));
    // The new set is allocated BEFORE the old one is released: if the device cannot hold both, the old table stays in
    // place, growth is switched off for this wgs_data and the run continues (an overflow is then reported as such).
    const Dev old = dev;
    d->mem.regroup(MemGroup::grid, MemGroup::old_grid);
    dev.cap = new_cap;
    dev.hmask = new_cap * 2u - 1u;
    if (alloc_grid(d) != WGS_OK) {
        d->mem.release_group(MemGroup::grid);
        d->mem.regroup(MemGroup::old_grid, MemGroup::grid);
        dev = old;
        d->auto_grow = false;
        hipGetLastError();  // (the failed allocation is not this call's error)
        return WGS_OK;
    }
    d->mem.release_group(MemGroup::old_grid);
    WGS_TRY(clear_table(d, true));
    d->sub.prev_sorted = false;      // block ids start over: the next substep bins every particle through the hash map
    d->sub.prebinned = false;        // (what the last G2P binned went with the old arrays)
    d->cdf_generation++;
    d->seen.ncpic = UINT32_MAX;
    d->seen.nvisit = UINT32_MAX;
    d->stats.grid_grown++;
    return WGS_OK;
}

// Looks at the counters the LAST wgs_step call left in pinned host memory (no synchronisation: skipped while that copy
// is still in flight) and keeps the table comfortable: more than half of the capacity active -> double it; more than
// three quarters of the ids handed out (blocks that were active at some point since the last rebuild) -> rebuild at
// the next substep instead of waiting for the 64-substep period.
wgs_status maintain_grid(wgs_data *d) {
    if (!d->seen.watch || !d->seen.watch_pending) return WGS_OK;
    if (hipEventQuery(d->seen.watch_event) != hipSuccess) {
        // the host runs ahead of the device: let it, for two calls; then wait for the copy (a bounded run-ahead keeps
        // the observation fresh enough to act before the table fills)
        if (++d->seen.watch_skips < 2u) return WGS_OK;
        HIP_TRY(hipEventSynchronize(d->seen.watch_event));
    }
    d->seen.watch_skips = 0;
    d->seen.watch_pending = false;
    const uint32_t nblocks = d->seen.watch[CTR_NBLOCKS], nphys = d->seen.watch[CTR_NPHYS], cap = d->dev.cap;
    if (d->dev.sharded) d->seen.nv_hint = std::max(d->seen.watch[CTR_NV], d->seen.watch[CTR_NV + CTR_SET]);
    // The observation is up to three calls old (two skips + the call that made it): a scene that is growing is judged by
    // where it will be by then at the rate of its last two observations, not by where it was.
    const uint32_t rate = nblocks > d->seen.nblocks && d->seen.nblocks != 0u ? nblocks - d->seen.nblocks : 0u;
    d->seen.nblocks = std::min(nblocks, cap);
    // (half full: grow, as before; or on course to be three quarters full by the time the next look can act)
    const uint64_t ahead = (uint64_t)nblocks + 3ull * rate;
    if (d->auto_grow && (nblocks > cap / 2u || ahead > cap / 4u * 3u) && cap < (1u << 24)) {
        uint32_t new_cap = cap * 2u;
        while (ahead > new_cap / 4u * 3u && new_cap < (1u << 24)) new_cap *= 2u;
        return grow_grid(d, new_cap);
    }
    if (nphys > cap / 4u * 3u) d->seen.force_rehash = true;
    if (d->seen.watch[CTR_NTOMB] > cap / 2u) d->seen.force_refresh = true;   // (marks of evicted blocks: a quarter of the 2 x cap slots)
    return WGS_OK;
}

// leaves a copy of the device counters in pinned host memory for the next call's maintain_grid (asynchronous)
wgs_status watch_counters(wgs_data *d) {
    if (!d->seen.watch) {   // (the watch exists with its event or not at all: a failure leaves nothing behind for the next call)
        Pinned<uint32_t> watch;
        Event copied;
        WGS_TRY(watch.alloc(CTR_COUNT));
        WGS_TRY(copied.create(hipEventDisableTiming));
        d->seen.watch = std::move(watch);
        d->seen.watch_event = std::move(copied);
    }
    HIP_TRY(hipMemcpyAsync(d->seen.watch.get(), d->dev.counters, sizeof(uint32_t) * CTR_COUNT, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipEventRecord(d->seen.watch_event, d->stream));
    d->seen.watch_pending = true;
    return WGS_OK;
}

wgs_status fetch_counters(wgs_data *d) {
    uint32_t host[CTR_COUNT];
    HIP_TRY(hipMemcpyAsync(host, d->dev.counters, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    d->seen.sync_nblocks = host[CTR_NBLOCKS] < d->dev.cap ? host[CTR_NBLOCKS] : d->dev.cap;
    d->seen.nblocks = d->seen.sync_nblocks;
    // (the list counters of the last substep: the set of its parity, layout.h; epoch of substep number s = s, counted from 1)
    const uint32_t last_epoch = (uint32_t)d->substeps;
    d->seen.ncpic = 0;  // the eight lists together
    for (uint32_t k = 0; k < 8; k++) d->seen.ncpic += std::min(host[ctr_ncpic(k, last_epoch)], d->dev.cap);
    d->seen.ncpic = std::min(d->seen.ncpic, d->dev.cap);
    d->seen.nvisit = 0;  // the longest of the eight lists
    for (uint32_t k = 0; k < 8; k++) d->seen.nvisit = std::max(d->seen.nvisit, std::min(host[ctr_nvisit(k, last_epoch)], d->dev.visit_cap));
    uint32_t movers = 0u;   // (16 partial counts, each modulo 2^32: so is their sum)
    for (int k = 0; k < 16; k++) movers += host[CTR_MOVERS + 32 * k];
    d->stats.movers_total += (uint32_t)(movers - d->seen.movers);
    d->seen.movers = movers;
    d->seen.nphys = host[CTR_NPHYS];
    d->seen.nfree = host[CTR_NFREE];
    d->seen.ntomb = host[CTR_NTOMB];
    d->seen.errors |= host[CTR_ERRORS];
    if (host[CTR_NBLOCKS] > d->dev.cap) d->seen.errors |= ERRBIT_OVERFLOW;
    if (host[CTR_NPHYS] > d->dev.cap / 4u * 3u) d->seen.force_rehash = true;
    if (host[CTR_NTOMB] > d->dev.cap / 2u) d->seen.force_refresh = true;
    return WGS_OK;
}

wgs_status sticky_status(wgs_data *d) {
    if (d->seen.errors & ERRBIT_OVERFLOW)
        return fail(WGS_ERR_GRID_OVERFLOW, "sparse grid overflow: more active blocks than grid_capacity");
    if (d->seen.errors & ERRBIT_SHARD)
        return fail(WGS_ERR_INVALID_ARGUMENT, "sharded run: a message buffer or the particle capacity overflowed, a particle left the decomposition, or the ranks disagree on the uniform-material mode");
    if (d->seen.errors & ERRBIT_KEYRANGE)
        return fail(WGS_ERR_KEY_RANGE, "a particle left the packed block-key range (grid.wgsl:88-95)");
    if (d->seen.errors & ERRBIT_HANDOVER)
        return fail(WGS_ERR_HIP, "internal: a grid-update wave gave up waiting for a block's P2G slab (the sort's block totals and cell runs disagree)");
    if (d->seen.errors & ERRBIT_PCDF)
        return fail(WGS_ERR_HIP, "internal: a near-collider workgroup of P2G gave up waiting for the prologue waves of its launch and computed the particle cdf itself (results intact; the launch lost 0.2 s)");
    if (d->seen.errors & ERRBIT_MATERIAL)
        return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_uniform_material: a particle of this wgs_data carries other constants (mass, init_volume, lambda, mu)");
    return WGS_OK;
}

void resolve_timings(wgs_data *d) {
    if (!d->timing.pending) return;
    hipStreamSynchronize(d->stream);
    for (int p = 0; p < WGS_NUM_PASSES; p++) d->timing.ms[p] = 0.f;
    // marks: 0 start | 1 after sort | 2 after node cdf | 3 after particle cdf | 4 after p2g | 5 after grid update |
    //        6 after the fused g2p launch | 7 after its near-collider launch | 8 after integrate_bodies
    const int pass_of_mark[8] = {WGS_PASS_GRID_SORT,   WGS_PASS_GRID_UPDATE_CDF, WGS_PASS_G2P_CDF,          WGS_PASS_P2G,
                                 WGS_PASS_GRID_UPDATE, WGS_PASS_G2P,             WGS_PASS_PARTICLES_UPDATE, WGS_PASS_INTEGRATE_BODIES};
    d->timing.mark_overhead_ms = 0.f;
    for (int s = 0; s < d->timing.events.used; s++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, d->timing.events.ev[s][9], d->timing.events.ev[s][10]) == hipSuccess) d->timing.mark_overhead_ms += ms;
    }
    if (d->timing.events.used > 0) d->timing.mark_overhead_ms /= (float)d->timing.events.used;
    for (int s = 0; s < d->timing.events.used; s++)
        for (int m = 0; m < 8; m++) {
            if (m == 6 && !d->cpic) continue;  // no second G2P launch: the two marks are adjacent
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, d->timing.events.ev[s][m], d->timing.events.ev[s][m + 1]) == hipSuccess)
                d->timing.ms[pass_of_mark[m]] += ms;
        }
    // (the emitting launches of the call, in front of their substeps' first mark: the table rebuild they ask for is "grid sort" too)
    for (size_t m = 0; m + 1 < d->timing.emit_marks.size(); m += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, d->timing.emit_marks[m], d->timing.emit_marks[m + 1]) == hipSuccess) d->timing.ms[WGS_PASS_GRID_SORT] += ms;
    }
    d->timing.pending = false;
}

}  // namespace
