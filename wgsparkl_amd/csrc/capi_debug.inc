// capi_debug.inc — entry points for looking inside: the device-side diagnostics (launch sequence: kernels_diag.h
// diag_enqueue), the scan test hook, and the profile readers of WGS_ABLATE builds.

extern "C" {

wgs_status wgs_enqueue_diagnostics(wgs_data *d, uint32_t what, wgs_diagnostics *device_out) {
    WGS_TRY(enter(d, device_out != nullptr));
    return diag_enqueue(d, what, device_out);
}

wgs_status wgs_read_diagnostics(wgs_data *d, uint32_t what, wgs_diagnostics *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (!d->diag_out) WGS_TRY(dev_alloc(d, &d->diag_out, 1));
    if (!d->diag_host) WGS_TRY(d->diag_host.alloc(1));
    WGS_TRY(diag_enqueue(d, what, d->diag_out));
    WGS_TRY(download(d, d->diag_host.get(), d->diag_out, sizeof(wgs_diagnostics)));
    memcpy(out, d->diag_host.get(), sizeof(wgs_diagnostics));
    return WGS_OK;
}

// Test hook: the exclusive scan of launch 2 (kernels_sort.h scan_chunk: what replaces prefix_sum.wgsl) on caller
// data — values[i] plays the particle count of block i, every block active. The reference's own scan test vectors
// (src/grid/prefix_sum.rs:183-229) go through the HIP scan this way.
wgs_status wgs_debug_scan(wgs_pipeline *pipeline, const uint32_t *values, uint32_t n, uint32_t *out, uint32_t *total) {
    if (!pipeline || (!values && n) || (!out && n)) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > (1u << 25)) return fail(WGS_ERR_INVALID_ARGUMENT, "n out of range");
    HIP_TRY(hipSetDevice(pipeline->device));
    Dev dev{};
    dev.cap = std::max(1u, n);
    const uint32_t nscan = (dev.cap + SCAN_CHUNK - 1) / SCAN_CHUNK, epoch = 1u;
    Scratch<uint32_t> counters, stamp, acc, active, start;
    Scratch<unsigned long long> chunk_a, chunk_b, group_a, group_b;
    const size_t ngroup = (size_t)nscan * SORT_THREADS;
    if (counters.alloc(CTR_COUNT, true) != WGS_OK || stamp.alloc(dev.cap, true) != WGS_OK || acc.alloc(dev.cap, true) != WGS_OK ||
        active.alloc(dev.cap, true) != WGS_OK || start.alloc(dev.cap, true) != WGS_OK || chunk_a.alloc(nscan, true) != WGS_OK ||
        chunk_b.alloc(nscan, true) != WGS_OK || group_a.alloc(ngroup, true) != WGS_OK || group_b.alloc(ngroup, true) != WGS_OK)
        return fail(WGS_ERR_HIP, "out of device memory");
    dev.counters = counters.ptr; dev.block_stamp = stamp.ptr; dev.block_acc = acc.ptr; dev.active = active.ptr; dev.block_start = start.ptr;
    dev.chunk_a = chunk_a.ptr; dev.chunk_b = chunk_b.ptr; dev.group_a = group_a.ptr; dev.group_b = group_b.ptr;
    std::vector<uint32_t> ones(dev.cap, epoch);
    uint32_t ctr[CTR_COUNT] = {0};
    ctr[CTR_NPHYS] = n;
    hipError_t e = hipMemcpy(dev.counters, ctr, sizeof(ctr), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dev.block_stamp, ones.data(), sizeof(uint32_t) * dev.cap, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(dev.block_acc, values, sizeof(uint32_t) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_scan_only, dim3(nscan + std::min((n + 3u) / 4u + 1u, 2048u)), dim3(SORT_THREADS), 0, 0, dev, epoch, nscan);
        e = hipDeviceSynchronize();
    }
    if (e == hipSuccess && n) e = hipMemcpy(out, dev.block_start, sizeof(uint32_t) * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total) {
        unsigned long long t = 0;  // sum of the chunk totals (low words)
        std::vector<unsigned long long> ct(nscan);
        e = hipMemcpy(ct.data(), dev.chunk_b, sizeof(unsigned long long) * nscan, hipMemcpyDeviceToHost);
        for (auto v : ct) t += v & 0xffffffffull;
        *total = (uint32_t)t;
    }
    if (e != hipSuccess) return fail(WGS_ERR_HIP, hipGetErrorString(e));
    return WGS_OK;
}

#ifdef WGS_ABLATE
// stage clocks of the fused G2P, of P2G and of launch 2 of the sort (kernels_transfer.h g_g2p_prof / g_p2g_prof, kernels_sort.h
// g_prof): read and reset. Experiment builds only, not in the header. `out` holds rows * 8 values.
static wgs_status read_and_reset_prof(const void *symbol, unsigned long long *out, size_t rows) {
    const std::vector<unsigned long long> zero(rows * 8, 0ull);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, symbol, sizeof(unsigned long long) * zero.size()));
    HIP_TRY(hipMemcpyToSymbol(symbol, zero.data(), sizeof(unsigned long long) * zero.size()));
    return WGS_OK;
}
wgs_status wgs_debug_g2p_prof(unsigned long long *out) { return read_and_reset_prof(HIP_SYMBOL(g_g2p_prof), out, WGS_G2P_ROWS); }
wgs_status wgs_debug_p2g_prof(unsigned long long *out) { return read_and_reset_prof(HIP_SYMBOL(g_p2g_prof), out, WGS_P2G_ROWS); }
wgs_status wgs_debug_prof(unsigned long long *out) { return read_and_reset_prof(HIP_SYMBOL(g_prof), out, WGS_PROF_ROWS); }
#endif

}  // extern "C"
