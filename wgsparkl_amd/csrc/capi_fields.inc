// capi_fields.inc — entry points of the Lagrangian field output: stress, invariants, volume ratio and stretches of every
// particle's stored state (wgs_read_particle_fields[_device]). The kernel is in kernels_fields.h. The _device form only
// enqueues on the data's stream; the host form stages through a Scratch and ends in download(), like the readers of
// capi_io.inc. Neither writes simulation state, touches Dev or keeps device memory.

namespace {
// the same launch under WGS_PLASTICITY_SNOW on data with plastic state (capi_plasticity.inc: its kernel behind every other)
void launch_particle_fields_snow(wgs_data *d, dim3 blocks, float *device_out);
}

extern "C" {

wgs_status wgs_read_particle_fields_device(wgs_data *d, wgs_particle_field *device_out) {
    WGS_TRY(enter(d, device_out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "sharded wgs_data: use wgs_shard_export");
    static_assert(sizeof(wgs_particle_field) == sizeof(float) * FIELD_WORDS, "wgs_particle_field is FIELD_WORDS words");
    if (reinterpret_cast<uintptr_t>(device_out) % (sizeof(float) * FIELD_VEC) != 0)
        return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_read_particle_fields_device: device_out must be aligned to 16 bytes (2D: 8)");
    const uint32_t n = d->dev.n;
    if (n == 0) return WGS_OK;
    const uint32_t groups = (n + FIELD_THREADS - 1) / FIELD_THREADS;
    const dim3 blocks(std::min(groups, (uint32_t)grid_for(d, 8)));
    if (d->plastic && d->plasticity == WGS_PLASTICITY_SNOW) launch_particle_fields_snow(d, blocks, reinterpret_cast<float *>(device_out));
    else hipLaunchKernelGGL(k_particle_fields<D>, blocks, dim3(FIELD_THREADS), 0, d->stream, d->dev, d->side, reinterpret_cast<float *>(device_out));
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_read_particle_fields(wgs_data *d, wgs_particle_field *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "sharded wgs_data: use wgs_shard_export");
    const uint32_t n = d->dev.n;
    if (n == 0) return WGS_OK;
    Scratch<wgs_particle_field> tmp;
    WGS_TRY(tmp.alloc(n));
    WGS_TRY(wgs_read_particle_fields_device(d, tmp.ptr));
    return download(d, out, tmp.ptr, sizeof(wgs_particle_field) * (size_t)n);
}

}  // extern "C"
