// capi_forces.inc — force fields: the launch enqueue_finish puts behind the grid update and in front of the domain walls on data that
// has a field set (launch_grid_forces, declared in host_substep.inc), and the two entry points. The kernel is in kernels_forces.h.
// The fields live in the handle (wgs_data::forces) and travel as a kernel argument: no device memory, no upload, nothing in Dev.

namespace {

void launch_grid_forces(wgs_data *d) {
    static_assert(sizeof(wgs_force_field) == 68 && sizeof(ForceSet) == 4 + 68 * WGS_MAX_FORCE_FIELDS, "the fields are a 548-byte kernel argument in both dimensions");
    ForceSet w{};
    w.n = d->forces_n;
    for (uint32_t i = 0; i < d->forces_n; i++) {
        const wgs_force_field &f = d->forces[i];
        w.kind[i] = f.kind;
        w.falloff[i] = f.falloff;
        w.region[i] = f.region;
        w.strength[i] = f.strength;
        w.softening[i] = f.softening;
        // the axis of a 3D vortex: normalised once, in double, rounded once (validated: |vec| > 0 and finite)
        const double len = (D == 3 && f.kind == WGS_FORCE_VORTEX) ? std::sqrt((double)f.vec[0] * f.vec[0] + (double)f.vec[1] * f.vec[1] + (double)f.vec[2] * f.vec[2]) : 1.0;
        for (int k = 0; k < 3; k++) {
            w.center[i][k] = f.center[k];
            w.vec[i][k] = (float)((double)f.vec[k] / len);
            w.rcenter[i][k] = f.region_center[k];
            w.rhalf[i][k] = f.region_half[k];
        }
    }
    // one wave per active block as the host last saw them (the waves stride over whatever the list holds now)
    const uint32_t blocks = d->seen.nblocks ? d->seen.nblocks : d->dev.cap;
    const uint32_t wgs_n = std::max(64u, std::min((uint32_t)grid_for(d, WGS_GU_WG_PER_CU), (blocks + 3u) / 4u));
    hipLaunchKernelGGL(k_grid_forces<D>, dim3(wgs_n), dim3(256), 0, d->stream, d->dev, w);
}

// nullptr: the field is acceptable; else what is wrong with it
const char *force_field_problem(const wgs_force_field &f) {
    if (f.kind > WGS_FORCE_DRAG) return "wgs_set_force_fields: kind must be WGS_FORCE_NONE .. WGS_FORCE_DRAG";
    if (f.falloff > 3u) return "wgs_set_force_fields: falloff must be 0 .. 3";
    if (f.region > WGS_REGION_BALL) return "wgs_set_force_fields: region must be WGS_REGION_ALL .. WGS_REGION_BALL";
    if (f.kind == WGS_FORCE_NONE) return nullptr;
    bool finite = std::isfinite(f.strength) && std::isfinite(f.softening);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(f.center[k]) && std::isfinite(f.vec[k]) && std::isfinite(f.region_center[k]) && std::isfinite(f.region_half[k]);
    if (!finite) return "wgs_set_force_fields: every float of a field must be finite";
    if (f.softening < 0.f) return "wgs_set_force_fields: softening must be >= 0";
    const bool central = f.kind == WGS_FORCE_RADIAL || f.kind == WGS_FORCE_VORTEX;
    if (central && f.falloff > 0u && f.softening == 0.f) return "wgs_set_force_fields: a falloff > 0 needs a softening > 0 (the centre would be a pole)";
    if (f.kind == WGS_FORCE_DRAG && f.strength < 0.f) return "wgs_set_force_fields: the rate of a drag field must be >= 0";
    if (f.region == WGS_REGION_BALL && f.region_half[0] < 0.f) return "wgs_set_force_fields: the radius of a ball region must be >= 0";
    if (f.region == WGS_REGION_BOX)
        for (int k = 0; k < D; k++)
            if (f.region_half[k] < 0.f) return "wgs_set_force_fields: the half extents of a box region must be >= 0";
    if (D == 3 && f.kind == WGS_FORCE_VORTEX && f.vec[0] == 0.f && f.vec[1] == 0.f && f.vec[2] == 0.f) return "wgs_set_force_fields: the axis of a vortex must not be zero";
    return nullptr;
}

}  // namespace

extern "C" {

wgs_status wgs_set_force_fields(wgs_data *d, const wgs_force_field *fields, uint32_t n) {
    WGS_TRY(enter(d));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_force_fields: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    if (n > WGS_MAX_FORCE_FIELDS) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_force_fields: at most WGS_MAX_FORCE_FIELDS fields");
    if (n > 0 && !fields) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_force_fields: NULL fields with n > 0");
    bool any = false;
    for (uint32_t i = 0; i < n; i++) {
        if (const char *problem = force_field_problem(fields[i])) return fail(WGS_ERR_INVALID_ARGUMENT, problem);
        any |= fields[i].kind != WGS_FORCE_NONE;
    }
    for (uint32_t i = 0; i < WGS_MAX_FORCE_FIELDS; i++) d->forces[i] = i < n ? fields[i] : wgs_force_field{};
    d->forces_n = n;
    d->forces_set = any;
    return WGS_OK;
}

wgs_status wgs_get_force_fields(wgs_data *d, wgs_force_field *out, uint32_t *n) {
    WGS_TRY(enter(d, out != nullptr && n != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_force_fields: sharded wgs_data (a slab holds a part of the grid): single-domain data only");
    for (uint32_t i = 0; i < WGS_MAX_FORCE_FIELDS; i++) out[i] = d->forces[i];
    *n = d->forces_n;
    return WGS_OK;
}

}  // extern "C"
