// capi_remove.inc — particles removed at run time (include/wgsparkl_hip_remove.h): the host side of kernels_remove.h. What a sink must be
// (sink_problem), the pass every path shares — keep (by id) -> scan -> compact (finish_removal) —, shrank_to, the mirror of capi_emit.inc's
// grew_by, fire_sinks — which wgs_step asks in front of every substep of data that has sinks, ahead of fire_emitters (declared in
// host_substep.inc) — and the entry points. Everything a pass needs on the device is Scratch<> for the length of the call: sinks take no
// device memory of the handle. Survivors are gathered into the OTHER buffer and copied back (DESIGN.md 7g says why not flipped).

namespace {

// nullptr: acceptable; else what is wrong with it. `scheduled`: wgs_set_sinks, which reads the schedule fields
const char *sink_problem(const wgs_sink &k, bool scheduled) {
    if (k.region != (uint32_t)WGS_REGION_BOX && k.region != (uint32_t)WGS_REGION_BALL) return "region must be WGS_REGION_BOX or WGS_REGION_BALL";
    if (k.side > (uint32_t)WGS_SINK_OUTSIDE) return "side must be WGS_SINK_INSIDE or WGS_SINK_OUTSIDE";
    if (scheduled && k.period == 0u) return "period must be >= 1";
    for (int c = 0; c < D; c++)
        if (!std::isfinite(k.center[c])) return "center must be finite";
    const int nhalf = k.region == (uint32_t)WGS_REGION_BOX ? D : 1;
    for (int c = 0; c < nhalf; c++)
        if (!std::isfinite(k.half[c]) || k.half[c] < 0.f) return "half must be finite and >= 0";
    return nullptr;
}

// `kept` particles are left, in the front slots of the current buffer: the counts every launch gets, and what the next substep must not assume
void shrank_to(wgs_data *d, uint32_t kept) {
    d->dev.n = d->dev.nv = kept;
    d->seen.force_rehash = true;    // the next substep bins the whole buffer through the table (k_bin), in whatever order it stands
    d->sub.prev_sorted = false;     // ... which is no longer the sorted output of the last substep (begin_substep drops what its G2P pre-binned)
}

uint32_t remove_grid(uint32_t n) { return (n + 255u) / 256u; }

// The keep-scan: keep[n] -> new_index[n] and *total (device words), three launches on `s`. tile_sums: (n + REMOVE_TILE - 1) / REMOVE_TILE words.
void launch_keep_scan(hipStream_t s, const uint8_t *keep, uint32_t n, uint32_t *tile_sums, uint32_t *new_index, uint32_t *total) {
    const uint32_t ntiles = (n + REMOVE_TILE - 1u) / REMOVE_TILE;
    hipLaunchKernelGGL(k_remove_tile_sums<D>, dim3(ntiles), dim3(REMOVE_THREADS), 0, s, keep, n, tile_sums);
    hipLaunchKernelGGL(k_remove_scan_tiles<D>, dim3(1), dim3(REMOVE_THREADS), 0, s, tile_sums, ntiles, total);
    hipLaunchKernelGGL(k_remove_apply<D>, dim3(ntiles), dim3(REMOVE_THREADS), 0, s, keep, n, tile_sums, new_index);
}

// keep[id] of the n_old particles is on the device and `removed` > 0 of them go: scan, compact the by-id tables and the slots, shrink.
// `scanned_tiles`: the tile offsets of `keep` if the caller has scanned them already (the mask forms learn the count that way: only
// k_remove_apply is left to launch), or null. `kept_from` (host) / `kept_from_device`: who asked gets the old indices of the survivors.
// Waits for the stream before it returns (the scratch arrays end with the call).
wgs_status finish_removal(wgs_data *d, const uint8_t *keep, uint32_t removed, const uint32_t *scanned_tiles, uint32_t *kept_from, uint32_t *kept_from_device) {
    Dev &dev = d->dev;
    hipStream_t s = d->stream;
    const uint32_t n_old = dev.n, kept = n_old - removed;
    const uint32_t ntiles = (n_old + REMOVE_TILE - 1u) / REMOVE_TILE;
    // one scratch block of words: new_index | kept_from | tile sums | total | radius | dp | phase | flags
    Scratch<uint32_t> words;
    WGS_TRY(words.alloc((size_t)n_old * 12 + ntiles + 1));
    uint32_t *new_index = words.ptr, *from = new_index + n_old, *tile_sums = from + n_old, *total = tile_sums + ntiles;
    float *tables = reinterpret_cast<float *>(total + 1);
    const IdTables own{d->static_radius, d->static_dp, d->static_phase, d->static_flags};
    const IdTables tmp{tables, tables + n_old, tables + (size_t)n_old * 7, reinterpret_cast<uint32_t *>(tables + (size_t)n_old * 9)};
    if (scanned_tiles) hipLaunchKernelGGL(k_remove_apply<D>, dim3(ntiles), dim3(REMOVE_THREADS), 0, s, keep, n_old, scanned_tiles, new_index);
    else launch_keep_scan(s, keep, n_old, tile_sums, new_index, total);
    hipLaunchKernelGGL(k_remove_tables<D>, dim3(remove_grid(n_old)), dim3(256), 0, s, own, tmp, n_old, keep, new_index, from);
    hipLaunchKernelGGL(k_remove_tables_back<D>, dim3(remove_grid(n_old)), dim3(256), 0, s, tmp, own, n_old, kept);
    hipLaunchKernelGGL(k_remove_compact<D>, dim3(remove_grid(n_old)), dim3(256), 0, s, dev, d->side, n_old, keep, new_index);
    hipLaunchKernelGGL(k_remove_settle<D>, dim3(remove_grid(n_old)), dim3(256), 0, s, dev, d->side, n_old, kept);
    HIP_TRY(hipGetLastError());
    if (kept_from && kept) HIP_TRY(hipMemcpyAsync(kept_from, from, sizeof(uint32_t) * (size_t)kept, hipMemcpyDeviceToHost, s));
    if (kept_from_device && kept) HIP_TRY(hipMemcpyAsync(kept_from_device, from, sizeof(uint32_t) * (size_t)kept, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    shrank_to(d, kept);
    return WGS_OK;
}

// nothing goes: the survivors are everybody
wgs_status kept_from_identity(wgs_data *d, uint32_t *kept_from, uint32_t *kept_from_device) {
    const uint32_t n = d->dev.n;
    if (kept_from)
        for (uint32_t i = 0; i < n; i++) kept_from[i] = i;
    if (kept_from_device && n) {
        std::vector<uint32_t> ids(n);
        for (uint32_t i = 0; i < n; i++) ids[i] = i;
        HIP_TRY(hipMemcpyAsync(kept_from_device, ids.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
    }
    return WGS_OK;
}

// The mask forms. `remove`: n bytes by id, in host (`on_device` false) or device memory.
wgs_status remove_by_mask(wgs_data *d, const uint8_t *remove, bool on_device, uint32_t *kept_from, uint32_t *kept_from_device, uint32_t *num_removed) {
    const uint32_t n = d->dev.n;
    *num_removed = 0;
    if (n == 0) return WGS_OK;
    WGS_TRY(enter(d));
    hipStream_t s = d->stream;
    const uint32_t ntiles = (n + REMOVE_TILE - 1u) / REMOVE_TILE;
    Scratch<uint8_t> keep;
    Scratch<uint32_t> count;   // tile sums | total (the first look: how many stay)
    WGS_TRY(keep.alloc(n));
    WGS_TRY(count.alloc((size_t)ntiles + 1));
    const uint8_t *mask = remove;
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(keep.ptr, remove, n, hipMemcpyHostToDevice, s));
        mask = keep.ptr;   // (in place: a thread reads and writes its own byte)
    }
    hipLaunchKernelGGL(k_remove_keep_of_mask<D>, dim3(remove_grid(n)), dim3(256), 0, s, mask, keep.ptr, n);
    hipLaunchKernelGGL(k_remove_tile_sums<D>, dim3(ntiles), dim3(REMOVE_THREADS), 0, s, keep.ptr, n, count.ptr);
    hipLaunchKernelGGL(k_remove_scan_tiles<D>, dim3(1), dim3(REMOVE_THREADS), 0, s, count.ptr, ntiles, count.ptr + ntiles);
    HIP_TRY(hipGetLastError());
    uint32_t kept = 0;
    WGS_TRY(download(d, &kept, count.ptr + ntiles, sizeof(uint32_t)));
    if (kept > n) return fail(WGS_ERR_HIP, "wgs_remove_particles: the keep-scan answered more particles than there are");
    if (kept == n) return kept_from_identity(d, kept_from, kept_from_device);
    WGS_TRY(finish_removal(d, keep.ptr, n - kept, count.ptr, kept_from, kept_from_device));
    *num_removed = n - kept;
    return WGS_OK;
}

// One pass over the regions of `set` (validated): mark, read the counts back — the stream waits —, and compact if some particle goes.
// taken[e]: particles region e took.
wgs_status remove_by_regions(wgs_data *d, const SinkSet &set, uint32_t *kept_from, uint32_t taken[WGS_MAX_SINKS], uint32_t *num_removed) {
    const uint32_t n = d->dev.n;
    *num_removed = 0;
    for (uint32_t e = 0; e < WGS_MAX_SINKS; e++) taken[e] = 0;
    if (n == 0 || set.n == 0) return kept_from_identity(d, kept_from, nullptr);
    hipStream_t s = d->stream;
    // ONE scratch block per pass, counts | keep: sinks own no device memory of the handle (wgs_stats.device_bytes), so a pass pays an
    // allocation and its release, which waits for the device (notes/round_35.md has the figure; the header states it)
    constexpr size_t COUNT_BYTES = sizeof(uint32_t) * WGS_MAX_SINKS;
    Scratch<uint8_t> block;
    WGS_TRY(block.alloc(COUNT_BYTES + n));
    uint32_t *counts = reinterpret_cast<uint32_t *>(block.ptr);
    uint8_t *keep = block.ptr + COUNT_BYTES;
    HIP_TRY(hipMemsetAsync(counts, 0, COUNT_BYTES, s));
    hipLaunchKernelGGL(k_remove_mark<D>, dim3((n + REMOVE_THREADS - 1u) / REMOVE_THREADS), dim3(REMOVE_THREADS), 0, s, d->dev, d->side, n, set, keep, counts);
    HIP_TRY(hipGetLastError());
    WGS_TRY(download(d, taken, counts, COUNT_BYTES));
    uint64_t removed = 0;
    for (uint32_t e = 0; e < set.n; e++) removed += taken[e];
    if (removed > n) return fail(WGS_ERR_HIP, "particle removal: the regions' counts exceed the particle count");
    if (removed == 0) return kept_from_identity(d, kept_from, nullptr);
    WGS_TRY(finish_removal(d, keep, (uint32_t)removed, nullptr, kept_from, nullptr));
    *num_removed = (uint32_t)removed;
    return WGS_OK;
}

// The sinks that are due in front of the substep about to be enqueued (the schedule of include/wgsparkl_hip_remove.h), in ONE pass.
// Host integers decide who is due; a pass waits for the stream once. A pass that takes nothing leaves everything as it was.
wgs_status fire_sinks(wgs_data *d, bool timed) {
    const uint64_t s = d->substeps;
    SinkSet due{};
    uint32_t slot_of[WGS_MAX_SINKS] = {};
    for (uint32_t e = 0; e < d->sink_n; e++) {
        const wgs_sink &k = d->sinks[e];
        if (s < k.start_substep || (s - k.start_substep) % k.period != 0u) continue;
        slot_of[due.n] = e;
        due.s[due.n++] = k;
    }
    if (due.n == 0 || d->dev.n == 0) return WGS_OK;
    Event before, after;
    if (timed) {
        WGS_TRY(before.create(hipEventDisableSystemFence));
        HIP_TRY(hipEventRecord(before, d->stream));
    }
    uint32_t taken[WGS_MAX_SINKS], removed = 0;
    WGS_TRY(remove_by_regions(d, due, nullptr, taken, &removed));
    for (uint32_t k = 0; k < due.n; k++) d->sink_removed[slot_of[k]] += taken[k];
    if (timed) {   // (a pair of marks like an emitting launch's: resolve_timings adds the interval to "grid sort")
        WGS_TRY(after.create(hipEventDisableSystemFence));
        HIP_TRY(hipEventRecord(after, d->stream));
        d->timing.emit_marks.push_back(std::move(before));
        d->timing.emit_marks.push_back(std::move(after));
    }
    return WGS_OK;
}

}  // namespace

extern "C" {

wgs_status wgs_remove_particles(wgs_data *d, const uint8_t *remove, uint32_t *kept_from, uint32_t *num_removed) {
    if (!d || !remove || !num_removed) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_remove_particles: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    return remove_by_mask(d, remove, false, kept_from, nullptr, num_removed);
}

wgs_status wgs_remove_particles_device(wgs_data *d, const uint8_t *remove_device, uint32_t *kept_from_device, uint32_t *num_removed) {
    if (!d || !remove_device || !num_removed) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_remove_particles_device: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    return remove_by_mask(d, remove_device, true, nullptr, kept_from_device, num_removed);
}

wgs_status wgs_remove_particles_in(wgs_data *d, const wgs_sink *regions, uint32_t n, uint32_t *kept_from, uint32_t *num_removed) {
    if (!d || !num_removed || (n > 0 && !regions)) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_remove_particles_in: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    if (n > WGS_MAX_SINKS) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_remove_particles_in: at most WGS_MAX_SINKS regions");
    SinkSet set{};
    for (uint32_t i = 0; i < n; i++) {
        if (const char *problem = sink_problem(regions[i], false))
            return fail(WGS_ERR_INVALID_ARGUMENT, std::string("wgs_remove_particles_in: ") + problem + " (region " + std::to_string(i) + ")");
        set.s[i] = regions[i];
    }
    set.n = n;
    WGS_TRY(enter(d));
    uint32_t taken[WGS_MAX_SINKS];
    return remove_by_regions(d, set, kept_from, taken, num_removed);
}

wgs_status wgs_set_sinks(wgs_data *d, const wgs_sink *sinks, uint32_t n) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_sinks: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    if (n > WGS_MAX_SINKS) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_sinks: at most WGS_MAX_SINKS sinks");
    if (n > 0 && !sinks) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_sinks: NULL sinks with n > 0");
    for (uint32_t i = 0; i < n; i++)
        if (const char *problem = sink_problem(sinks[i], true))
            return fail(WGS_ERR_INVALID_ARGUMENT, std::string("wgs_set_sinks: ") + problem + " (sink " + std::to_string(i) + ")");
    for (uint32_t i = 0; i < WGS_MAX_SINKS; i++) {
        d->sinks[i] = i < n ? sinks[i] : wgs_sink{};
        d->sink_removed[i] = 0;
    }
    d->sink_n = n;
    d->sinks_set = n > 0;
    return WGS_OK;
}

wgs_status wgs_get_sinks(wgs_data *d, wgs_sink *out, uint32_t *n) {
    if (!d || !out || !n) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_sinks: sharded wgs_data: single-domain data only");
    for (uint32_t i = 0; i < WGS_MAX_SINKS; i++) out[i] = d->sinks[i];
    *n = d->sink_n;
    return WGS_OK;
}

wgs_status wgs_get_sink_counts(wgs_data *d, uint64_t removed[WGS_MAX_SINKS]) {
    if (!d || !removed) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_sink_counts: sharded wgs_data: single-domain data only");
    for (uint32_t i = 0; i < WGS_MAX_SINKS; i++) removed[i] = d->sink_removed[i];
    return WGS_OK;
}

wgs_status wgs_debug_compact_map(wgs_pipeline *pipeline, const uint8_t *remove, uint32_t n, uint32_t *new_index, uint32_t *kept) {
    if (!pipeline || (n && (!remove || !new_index))) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > (1u << 28)) return fail(WGS_ERR_INVALID_ARGUMENT, "n out of range");
    if (n == 0) {
        if (kept) *kept = 0;
        return WGS_OK;
    }
    HIP_TRY(hipSetDevice(pipeline->device));
    const uint32_t ntiles = (n + REMOVE_TILE - 1u) / REMOVE_TILE;
    Scratch<uint8_t> keep;
    Scratch<uint32_t> words;   // new_index | tile sums | total
    WGS_TRY(keep.alloc(n));
    WGS_TRY(words.alloc((size_t)n + ntiles + 1));
    HIP_TRY(hipMemcpy(keep.ptr, remove, n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_remove_keep_of_mask<D>, dim3(remove_grid(n)), dim3(256), 0, 0, keep.ptr, keep.ptr, n);
    launch_keep_scan(0, keep.ptr, n, words.ptr + n, words.ptr, words.ptr + n + ntiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(new_index, words.ptr, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (kept) HIP_TRY(hipMemcpy(kept, words.ptr + n + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return WGS_OK;
}

}  // extern "C"
