// capi_probe.inc — entry points of the Eulerian field output: the grid of the last substep sampled at arbitrary points
// (wgs_sample_grid[_device]) and a dense window of its nodes (wgs_read_grid_window[_device]). The kernels are in
// kernels_probe.h. The _device forms only enqueue on the data's stream; the host forms stage through a Scratch and end in
// download(), like the readers of capi_io.inc. None of them writes simulation state or touches Dev.

namespace {

// the sampler's scratch word per block id (kernels_probe.h k_probe_mark): allocated by the first call, replaced when the
// block capacity has grown since; returns the ticket of this call
wgs_status probe_marks(wgs_data *d, uint32_t *ticket) {
    if (!d->probe_mark || d->probe_mark_cap != d->dev.cap) {
        if (d->probe_mark) {
            HIP_TRY(hipStreamSynchronize(d->stream));   // (an earlier sampler may still read the old words)
            d->mem.release(d->probe_mark);
            d->probe_mark = nullptr;
        }
        WGS_TRY(dev_alloc(d, &d->probe_mark, d->dev.cap));   // (zeroed on the stream: no ticket is 0)
        d->probe_mark_cap = d->dev.cap;
    }
    if (++d->probe_ticket == 0u) {   // 2^32 calls: start over on cleared words
        HIP_TRY(hipMemsetAsync(d->probe_mark, 0, sizeof(uint32_t) * (size_t)d->dev.cap, d->stream));
        d->probe_ticket = 1u;
    }
    *ticket = d->probe_ticket;
    return WGS_OK;
}

wgs_status probe_window_args(const int32_t *lo, const uint32_t *dims, size_t *nodes) {
    if (!lo || !dims) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long total = 1ull;
    for (int k = 0; k < D; k++) {
        if (dims[k] == 0u) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_read_grid_window: every dims[k] must be at least 1");
        total *= dims[k];
        if (total >= (1ull << 31)) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_read_grid_window: the product of dims must be below 2^31");
    }
    *nodes = (size_t)total;
    return WGS_OK;
}

}  // namespace

extern "C" {

wgs_status wgs_sample_grid_device(wgs_data *d, const float *device_points, size_t n, wgs_grid_sample *device_out) {
    WGS_TRY(enter(d, (device_points && device_out) || n == 0));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_sample_grid: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    static_assert(sizeof(wgs_grid_sample) == sizeof(float) * PROBE_WORDS, "wgs_grid_sample is PROBE_WORDS words");
    if (n == 0) return WGS_OK;
    if (n > 0x7fffffffull) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_sample_grid: more than 2^31 - 1 points in one call");
    uint32_t ticket = 0u;
    WGS_TRY(probe_marks(d, &ticket));
    hipLaunchKernelGGL(k_probe_mark<D>, dim3(grid_for(d, 1)), dim3(256), 0, d->stream, d->dev, d->probe_mark, ticket);
    const uint32_t groups = (uint32_t)((n + PROBE_THREADS - 1) / PROBE_THREADS);
    hipLaunchKernelGGL(k_probe_sample<D>, dim3(std::min(groups, (uint32_t)grid_for(d, 8))), dim3(PROBE_THREADS), 0, d->stream, d->dev,
                       (const uint32_t *)d->probe_mark, ticket, device_points, (uint32_t)n, reinterpret_cast<float *>(device_out));
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_sample_grid(wgs_data *d, const float *points, size_t n, wgs_grid_sample *out) {
    WGS_TRY(enter(d, (points && out) || n == 0));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_sample_grid: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    if (n == 0) return WGS_OK;
    if (n > 0x7fffffffull) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_sample_grid: more than 2^31 - 1 points in one call");
    Scratch<float> pts;
    Scratch<wgs_grid_sample> tmp;
    WGS_TRY(pts.alloc(n * D));
    WGS_TRY(tmp.alloc(n));
    HIP_TRY(hipMemcpyAsync(pts.ptr, points, sizeof(float) * n * D, hipMemcpyHostToDevice, d->stream));
    WGS_TRY(wgs_sample_grid_device(d, pts.ptr, n, tmp.ptr));
    return download(d, out, tmp.ptr, sizeof(wgs_grid_sample) * n);
}

wgs_status wgs_read_grid_window_device(wgs_data *d, const int32_t *lo, const uint32_t *dims, float *device_out) {
    WGS_TRY(enter(d, device_out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_read_grid_window: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    size_t nodes = 0;
    WGS_TRY(probe_window_args(lo, dims, &nodes));
    ProbeWindow win{};
    for (int k = 0; k < D; k++) { win.lo[k] = lo[k]; win.dims[k] = dims[k]; }
    HIP_TRY(hipMemsetAsync(device_out, 0, sizeof(float) * (D + 1) * nodes, d->stream));
    hipLaunchKernelGGL(k_probe_window<D>, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, win, device_out);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_read_grid_window(wgs_data *d, const int32_t *lo, const uint32_t *dims, float *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_read_grid_window: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    size_t nodes = 0;
    WGS_TRY(probe_window_args(lo, dims, &nodes));
    Scratch<float> tmp;
    WGS_TRY(tmp.alloc(nodes * (D + 1)));
    WGS_TRY(wgs_read_grid_window_device(d, lo, dims, tmp.ptr));
    return download(d, out, tmp.ptr, sizeof(float) * (D + 1) * nodes);
}

}  // extern "C"
