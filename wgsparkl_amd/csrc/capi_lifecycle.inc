// capi_lifecycle.inc — entry points that make, advance and end a simulation: library info, pipeline and data create /
// destroy (create_impl stages and uploads the particles), wgs_set_stream, wgs_step, wgs_sync.

namespace {

uint32_t next_pow2(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

void fill_collider(ColliderDev &c, const wgs_collider &in) {
    c.shape_type = in.shape_type;
    for (int k = 0; k < 4; k++) c.shape[k] = in.shape[k];
    for (int k = 0; k < 4; k++) c.rot[k] = in.pose.rotation[k];
    for (int k = 0; k < 3; k++) c.trans[k] = in.pose.translation[k];
    c.scale = in.pose.scale;
    for (int k = 0; k < 3; k++) c.linvel[k] = in.velocity.linear[k];
    for (int k = 0; k < 3; k++) c.angvel[k] = in.velocity.angular[k];
    for (int k = 0; k < 3; k++) c.com[k] = in.com[k];
}

}  // namespace

extern "C" {

const char *wgs_last_error(void) { return g_last_error.c_str(); }
int32_t wgs_dim(void) { return D; }
uint32_t wgs_abi_version(void) { return WGS_ABI_VERSION; }
const char *wgs_build_info(void) {
    return "wgsparkl_hip dim=" WGS_STR(WGS_DIM) " arch=gfx950"
#ifdef WGS_ABLATE
           " WGS_ABLATE"
#endif
        ;
}

wgs_status wgs_pipeline_create(int32_t hip_device, wgs_pipeline **out) {
    if (!out) return fail(WGS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(WGS_ERR_NO_DEVICE, std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (hip_device < 0 || hip_device >= count) return fail(WGS_ERR_INVALID_ARGUMENT, "hip_device out of range");
    HIP_TRY(hipSetDevice(hip_device));
    wgs_pipeline *p = new wgs_pipeline();
    p->device = hip_device;
    {
        const hipError_t pe = hipGetDeviceProperties(&p->props, hip_device);
        if (pe != hipSuccess) {
            delete p;
            return fail(WGS_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(pe));
        }
    }
    p->num_cus = p->props.multiProcessorCount > 0 ? p->props.multiProcessorCount : 256;
    *out = p;
    return WGS_OK;
}

void wgs_pipeline_destroy(wgs_pipeline *pipeline) { delete pipeline; }

static wgs_status create_impl(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                              size_t num_particles, const uint32_t *global_ids, const wgs_collider *colliders,
                              size_t num_colliders, float cell_width, uint32_t grid_capacity, size_t particle_capacity,
                              bool sharded, int32_t block_lo, int32_t block_hi, int32_t force_plastic, wgs_data **out) {
    if (!pipeline || !params || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (num_particles && !particles) return fail(WGS_ERR_INVALID_ARGUMENT, "particles is NULL");
    if (num_colliders && !colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "colliders is NULL");
    if (num_colliders > WGS_MAX_COLLIDERS)
        return fail(WGS_ERR_UNSUPPORTED, "at most 16 coupled colliders (grid.wgsl:230-240)");
    if (!(cell_width > 0.f)) return fail(WGS_ERR_INVALID_ARGUMENT, "cell_width must be > 0");
    if (grid_capacity == 0 || grid_capacity > (1u << 25)) return fail(WGS_ERR_INVALID_ARGUMENT, "grid_capacity out of range");
    // 32-bit byte offsets inside one ping-pong buffer (layout.h ldp/stp)
    if (particle_capacity < num_particles) particle_capacity = num_particles;
    if (buffer_floats<D>((uint32_t)particle_capacity + 64) * 4 >= (1ull << 32))
        return fail(WGS_ERR_UNSUPPORTED, "more than ~21M particles per wgs_data: shard across GPUs");
    *out = nullptr;
    HIP_TRY(hipSetDevice(pipeline->device));
    // (destroyed on every return but the last one, which hands it to the caller)
    std::unique_ptr<wgs_data, void (*)(wgs_data *)> guard(new wgs_data(), wgs_data_destroy);
    wgs_data *d = guard.get();
    d->pipeline = pipeline;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(WGS_ERR_HIP, "hipStreamCreate failed");
    Dev &dev = d->dev;
    const uint32_t n = (uint32_t)num_particles;
    dev.n = n;
    dev.nv = n;
    dev.sharded = sharded ? 1u : 0u;
    dev.shard_lo = sharded ? block_lo : INT32_MIN;
    dev.shard_hi = sharded ? block_hi : INT32_MAX;
    d->capacity = (uint32_t)particle_capacity;
    dev.npad = (((uint32_t)particle_capacity + 63u) / 64u) * 64u;
    if (dev.npad == 0) dev.npad = 64;
    dev.cap = next_pow2(grid_capacity);  // grid.rs:283
    dev.hmask = dev.cap * 2u - 1u;  // half-full table (reference: exactly cap slots, quirk B4)
    dev.h = cell_width;
    dev.inv_h = 1.0f / cell_width;
    {
        int e = 0;
        dev.h_pow2 = (frexpf(cell_width, &e) == 0.5f) ? 1u : 0u;
    }
    dev.model = WGS_MODEL_COROTATED;
    dev.fluid_gamma = 7.0f;   // (wgs_set_fluid_eos)
    // developer switches (layout.h DebugSwitch), read once, here; 0 in production
    dev.dbg = getenv("WGS_DEBUG") ? (uint32_t)strtoul(getenv("WGS_DEBUG"), nullptr, 0) : 0u;
    if (getenv("WGS_REHASH_PERIOD")) d->rehash_period = std::max(1u, (uint32_t)strtoul(getenv("WGS_REHASH_PERIOD"), nullptr, 0));  // same results
#ifndef WGS_ABLATE
    dev.dbg &= WGS_LAUNCH_SHAPE_SWITCHES;
#endif
    dev.n_colliders = (uint32_t)num_colliders;
    d->cpic = num_colliders > 0;

    // (the order of the allocations decides addresses, and addresses decide channel placement: keep it)
    const size_t plane_floats = buffer_floats<D>(dev.npad);
    WGS_TRY(dev_alloc(d, &dev.buf[0], plane_floats));
    WGS_TRY(dev_alloc(d, &dev.buf[1], plane_floats));
    WGS_TRY(dev_alloc(d, &dev.perm, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.perm_cell, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.cellid, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.mv_next, (size_t)dev.npad));
    WGS_TRY(alloc_grid(d));
    // data that evicts its long-inactive blocks needs no periodic table rebuild (the marks the evictions leave are cleared by
    // k_table_refresh, without touching a particle) — slabs of a decomposition included since round 6
    if (dev.free_ids != nullptr && !getenv("WGS_REHASH_PERIOD")) d->rehash_period = 0u;
    WGS_TRY(dev_alloc(d, &dev.counters, (size_t)CTR_COUNT));
    WGS_TRY(dev_alloc(d, &d->sp, (size_t)1));
    WGS_TRY(dev_alloc(d, &d->colliders, (size_t)WGS_MAX_COLLIDERS));
    WGS_TRY(dev_alloc(d, &dev.bodies, (size_t)WGS_MAX_COLLIDERS));
    WGS_TRY(dev_alloc(d, &dev.impulses, (size_t)WGS_MAX_COLLIDERS * 8));
    WGS_TRY(dev_alloc(d, &d->static_radius, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &d->static_dp, (size_t)dev.npad * 6));
    WGS_TRY(dev_alloc(d, &d->static_phase, (size_t)dev.npad * 2));
    WGS_TRY(dev_alloc(d, &d->static_flags, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &d->shard_counts, (size_t)4));
    if (sharded) {
        dev.leavers_cap = std::max<uint32_t>(4096u, (uint32_t)(particle_capacity / 16));
        WGS_TRY(dev_alloc(d, &dev.leavers, (size_t)dev.leavers_cap));
    }
    dev.sp = d->sp;
    dev.colliders = d->colliders;

    // AoS -> SoA staging (GpuParticles::from_particles + GpuModels::from_particles,
    // particle3d.rs:192-210, models/mod.rs:20-49).
    std::vector<float> soa(plane_floats, 0.f);
    std::vector<float> s_radius(dev.npad, 0.f), s_dp((size_t)dev.npad * 6, 0.f), s_phase((size_t)dev.npad * 2, 0.f);
    std::vector<uint32_t> s_flags(dev.npad, 0u);
    const float deg = 3.14159265358979323846f / 180.0f;
    const float default_dp[6] = {35.0f * deg, 9.0f * deg, 0.2f, 10.0f * deg, -1.0f, -1.0f};  // DruckerPrager::new(-1, -1)
    bool plastic = false;
    auto quad = [&](int qd, uint32_t i) { return soa.data() + ((size_t)qd * dev.npad + i) * 4; };
    uint32_t *pid_plane = reinterpret_cast<uint32_t *>(soa.data() + (size_t)P::NQ * 4 * dev.npad);
    for (uint32_t i = 0; i < n; i++) {
        const wgs_particle &q = particles[i];
        const wgs_particle_dynamics &dy = q.dynamics;
        float aff_bits;
        memcpy(&aff_bits, &dy.cdf.affinity, 4);
        if constexpr (D == 3) {
            using P3 = Pl<3>;
            float *p;
            p = quad(P3::XM, i); p[0] = q.position[0]; p[1] = q.position[1]; p[2] = q.position[D - 1]; p[3] = dy.mass;
            p = quad(P3::CV0, i); p[0] = dy.affine[0]; p[1] = dy.affine[1]; p[2] = dy.affine[2]; p[3] = dy.affine[3];
            p = quad(P3::CV0 + 1, i); p[0] = dy.affine[DD - 5]; p[1] = dy.affine[DD - 4]; p[2] = dy.affine[DD - 3]; p[3] = dy.affine[DD - 2];
            p = quad(P3::CV2, i); p[0] = dy.affine[DD - 1]; p[1] = dy.velocity[0]; p[2] = dy.velocity[1]; p[3] = dy.velocity[D - 1];
            p = quad(P3::F0, i); p[0] = dy.def_grad[0]; p[1] = dy.def_grad[1]; p[2] = dy.def_grad[2]; p[3] = dy.def_grad[3];
            p = quad(P3::F0 + 1, i); p[0] = dy.def_grad[DD - 5]; p[1] = dy.def_grad[DD - 4]; p[2] = dy.def_grad[DD - 3]; p[3] = dy.def_grad[DD - 2];
            p = quad(P3::F0 + 2, i); p[0] = dy.def_grad[DD - 1]; p[1] = dy.init_volume; p[2] = q.model.lambda; p[3] = q.model.mu;
            p = quad(P3::CDF0, i); p[0] = dy.cdf.normal[0]; p[1] = dy.cdf.normal[1]; p[2] = dy.cdf.normal[D - 1]; p[3] = dy.cdf.signed_distance;
            p = quad(P3::CDF1, i); p[0] = dy.cdf.rigid_vel[0]; p[1] = dy.cdf.rigid_vel[1]; p[2] = dy.cdf.rigid_vel[D - 1]; p[3] = aff_bits;
        } else {
            using P2 = Pl<2>;
            float *p;
            p = quad(P2::XM, i); p[0] = q.position[0]; p[1] = q.position[1]; p[2] = dy.mass; p[3] = dy.init_volume;
            p = quad(P2::CV0, i); p[0] = dy.affine[0]; p[1] = dy.affine[1]; p[2] = dy.affine[2]; p[3] = dy.affine[3];
            p = quad(P2::CV2, i); p[0] = dy.velocity[0]; p[1] = dy.velocity[1]; p[2] = q.model.lambda; p[3] = q.model.mu;
            p = quad(P2::F0, i); p[0] = dy.def_grad[0]; p[1] = dy.def_grad[1]; p[2] = dy.def_grad[2]; p[3] = dy.def_grad[3];
            p = quad(P2::CDF0, i); p[0] = dy.cdf.normal[0]; p[1] = dy.cdf.normal[1]; p[2] = dy.cdf.signed_distance; p[3] = aff_bits;
            p = quad(P2::CDF1, i); p[0] = dy.cdf.rigid_vel[0]; p[1] = dy.cdf.rigid_vel[1]; p[2] = 0.f; p[3] = 0.f;
        }
        pid_plane[i] = global_ids ? global_ids[i] : i;
        const float *dp = q.has_plasticity ? &q.plasticity.h0 : default_dp;
        const float phase = q.has_phase ? q.phase.phase : 0.0f;            // models/mod.rs:33-36
        const float max_stretch = q.has_phase ? q.phase.max_stretch : -1.0f;
        {
            float *p;
            p = quad(P::DP0, i); p[0] = dp[0]; p[1] = dp[1]; p[2] = dp[2]; p[3] = dp[3];
            // DruckerPragerPlasticState::default() = {1, 1, 0}, drucker_prager.rs:44-53
            p = quad(P::DP1, i); p[0] = dp[4]; p[1] = dp[5]; p[2] = 1.0f; p[3] = 1.0f;
            p = quad(P::DP2, i); p[0] = 0.0f; p[1] = phase; p[2] = max_stretch; p[3] = 0.f;
        }
        for (int k = 0; k < 6; k++) s_dp[(size_t)i * 6 + k] = dp[k];
        s_phase[(size_t)i * 2] = phase;
        s_phase[(size_t)i * 2 + 1] = max_stretch;
        s_radius[i] = q.dynamics.init_radius;
        s_flags[i] = (q.has_plasticity ? 1u : 0u) | (q.has_phase ? 2u : 0u);
        // Does the plasticity / fracture branch ever run for this particle?
        // (particle_update.wgsl:98-122; max_stretch >= FLT_MAX can never be exceeded by a finite F)
        if ((phase == 0.0f && dp[4] != 0.0f) || (phase > 0.0f && max_stretch > 0.0f && max_stretch < FLT_MAX)) plastic = true;
    }
    d->plastic = plastic || force_plastic != 0;
    // uniform plasticity parameters (bitwise; single-domain data, like the automatic uniform-material mode; layout.h Dev::uni_dp):
    // 1 = one set of h0..h3, 2 = all six and max_stretch — the per-particle state is then packed into DP1 before the upload
    if (d->plastic && n > 0 && !sharded && !(dev.dbg & DBG_NO_UNIFORM)) {
        bool u4 = true, u6 = true;
        for (uint32_t i = 1; i < n && u4; i++) {
            u4 = memcmp(&s_dp[(size_t)i * 6], &s_dp[0], 4 * sizeof(float)) == 0;
            u6 = u6 && memcmp(&s_dp[(size_t)i * 6 + 4], &s_dp[4], 2 * sizeof(float)) == 0 && memcmp(&s_phase[(size_t)i * 2 + 1], &s_phase[1], sizeof(float)) == 0;
        }
        if (u4) {
            dev.uni_dp = u6 ? 2u : 1u;
            for (int k = 0; k < 6; k++) dev.uni_dpv[k] = s_dp[k];
            dev.uni_max_stretch = s_phase[1];
            if (u6)
                for (uint32_t i = 0; i < n; i++) {
                    float *q1 = quad(P::DP1, i);
                    const float *q2 = quad(P::DP2, i);
                    q1[0] = q1[2]; q1[1] = q1[3]; q1[2] = q2[0]; q1[3] = q2[1];   // (st0, st1, st2, phase)
                }
        }
    }
    // one material for all particles (bitwise)? -> uniform-material mode (layout.h). Sharded data: the caller says so
    // (wgs_set_uniform_material), a rank cannot know the other ranks' particles.
    bool uniform = D == 3 && n > 0 && !sharded && !(dev.dbg & DBG_NO_UNIFORM);
    for (uint32_t i = 1; i < n && uniform; i++)
        uniform = memcmp(&particles[i].dynamics.mass, &particles[0].dynamics.mass, 4) == 0 &&
                  memcmp(&particles[i].dynamics.init_volume, &particles[0].dynamics.init_volume, 4) == 0 &&
                  memcmp(&particles[i].model, &particles[0].model, sizeof(wgs_elastic_coefficients)) == 0;
    auto h2d = [&](void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream) == hipSuccess ? WGS_OK : fail(WGS_ERR_HIP, "hipMemcpy H2D failed");
    };
    WGS_TRY(h2d(dev.buf[0], soa.data(), plane_floats * sizeof(float)));
    WGS_TRY(h2d(d->static_radius, s_radius.data(), s_radius.size() * sizeof(float)));
    WGS_TRY(h2d(d->static_dp, s_dp.data(), s_dp.size() * sizeof(float)));
    WGS_TRY(h2d(d->static_phase, s_phase.data(), s_phase.size() * sizeof(float)));
    WGS_TRY(h2d(d->static_flags, s_flags.data(), s_flags.size() * sizeof(uint32_t)));
    d->host_sp = SimParamsDev{};
    fill_sim_params(d->host_sp, params);
    WGS_TRY(h2d(d->sp, &d->host_sp, sizeof(SimParamsDev)));
    if (sharded) {
        // counts live on the device; the host-side n / nv become the launch bound (allocated capacity)
        uint32_t cnt[2] = {n, n};
        WGS_TRY(h2d(dev.counters + CTR_N, cnt, sizeof(cnt)));
        WGS_TRY(h2d(dev.counters + CTR_N + CTR_SET, cnt, sizeof(cnt)));   // (both sets: layout.h ctr_cur / ctr_next)
        dev.n = dev.nv = (uint32_t)particle_capacity;
        d->seen.nv_hint = n;
    }
    d->host_colliders.resize(WGS_MAX_COLLIDERS);
    memset(d->host_colliders.data(), 0, sizeof(ColliderDev) * WGS_MAX_COLLIDERS);
    for (size_t i = 0; i < num_colliders; i++) fill_collider(d->host_colliders[i], colliders[i]);
    WGS_TRY(h2d(d->colliders, d->host_colliders.data(), sizeof(ColliderDev) * WGS_MAX_COLLIDERS));
    d->host_bodies.assign(WGS_MAX_COLLIDERS, BodyDev{});
    note_moving(d, moving_by_velocity(d, num_colliders));
    if (num_colliders)  // local centres of mass from the world ones (update_world_mass_properties' inverse)
        hipLaunchKernelGGL(k_bodies_refresh<D>, dim3(1), dim3(16), 0, d->stream, dev, 0xffffu);
    if (d->bodies_move && enable_impulses(d) != WGS_OK) return fail(WGS_ERR_HIP, "out of device memory for the impulse accumulators");
    if (uniform) {
        dev.uniform = 1u;
        dev.uni_mass = particles[0].dynamics.mass;
        dev.uni_vol = particles[0].dynamics.init_volume;
        dev.uni_lambda = particles[0].model.lambda;
        dev.uni_mu = particles[0].model.mu;
        hipLaunchKernelGGL(k_to_uniform, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, dev, 0, 0);
    }
    if (dev.uni_dp != 0u) {   // (the other ping-pong buffer's copy of the quads the step leaves alone: layout.h Dev::uni_dp)
        for (int qd : {(int)Pl<D>::DP0, (int)Pl<D>::DP2}) {
            const size_t plane = (size_t)qd * dev.npad * 4;   // (floats: quad q of slot i sits at float (q * npad + i) * 4)
            if (hipMemcpyAsync(dev.buf[1] + plane, dev.buf[0] + plane, (size_t)dev.npad * 16, hipMemcpyDeviceToDevice, d->stream) != hipSuccess)
                return fail(WGS_ERR_HIP, "hipMemcpy D2D failed");
        }
    }
    if (hipStreamSynchronize(d->stream) != hipSuccess) return fail(WGS_ERR_HIP, "initial upload failed");
    *out = guard.release();
    return WGS_OK;
}

wgs_status wgs_data_create(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                           size_t num_particles, const wgs_collider *colliders, size_t num_colliders, float cell_width,
                           uint32_t grid_capacity, wgs_data **out) {
    return create_impl(pipeline, params, particles, num_particles, nullptr, colliders, num_colliders, cell_width,
                       grid_capacity, num_particles, false, 0, 0, 0, out);
}

wgs_status wgs_data_create_sharded(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                                   size_t num_particles, const uint32_t *global_ids, const wgs_collider *colliders,
                                   size_t num_colliders, float cell_width, uint32_t grid_capacity,
                                   uint32_t particle_capacity, int32_t block_lo, int32_t block_hi, int32_t force_plastic,
                                   wgs_data **out) {
    if (block_lo >= block_hi) return fail(WGS_ERR_INVALID_ARGUMENT, "empty shard range");
    return create_impl(pipeline, params, particles, num_particles, global_ids, colliders, num_colliders, cell_width,
                       grid_capacity, particle_capacity, true, block_lo, block_hi, force_plastic, out);
}

wgs_status wgs_set_stream(wgs_data *d, void *hip_stream) {
    WGS_TRY(enter(d, true, "data is NULL"));
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (d->owns_stream && d->stream) HIP_TRY(hipStreamDestroy(d->stream));
    d->stream = static_cast<hipStream_t>(hip_stream);
    d->owns_stream = false;
    return WGS_OK;
}

void wgs_data_destroy(wgs_data *d) {
    if (!d) return;
    if (d->stream) hipStreamSynchronize(d->stream);
    if (d->timing.events.created)
        for (int s = 0; s < Events::MAX_SUBSTEPS; s++)
            for (int m = 0; m < Events::MARKS; m++) hipEventDestroy(d->timing.events.ev[s][m]);
    d->mem.release_all();
    if (d->stream && d->owns_stream) hipStreamDestroy(d->stream);
    if (d->seen.watch) hipHostFree(d->seen.watch);
    if (d->diag_host) hipHostFree(d->diag_host);
    if (d->seen.watch_event) hipEventDestroy(d->seen.watch_event);
    delete d->link;
    delete d;
}

wgs_status wgs_step(wgs_pipeline *pipeline, wgs_data *d, uint32_t num_substeps, int32_t timestamps) {
    WGS_TRY(enter(d, pipeline != nullptr));
    if (timestamps) {
        if (!d->timing.events.created) {
            for (int s = 0; s < Events::MAX_SUBSTEPS; s++)
                for (int m = 0; m < Events::MARKS; m++) HIP_TRY(hipEventCreateWithFlags(&d->timing.events.ev[s][m], hipEventDisableSystemFence));  // timing only: no cache writeback per mark
            d->timing.events.created = true;
        }
        d->timing.events.used = 0;
    }
    WGS_TRY(maintain_grid(d));
    auto flush_bodies = [&]() {   // the last substep's integrate_bodies: every other entry point finds the bodies integrated
        if (d->sub.bodies_pending) launch_bodies_integrate(d);
        d->sub.bodies_pending = false;
    };
    for (uint32_t i = 0; i < num_substeps; i++) {
        wgs_status st = WGS_OK;
        if (i > 0 && i % 64u == 0u) {  // long calls: keep an eye on the table inside the call too (bounded run-ahead)
            if ((st = watch_counters(d)) == WGS_OK) st = maintain_grid(d);
        }
        // (a whole substep: the four stages of host_substep.inc; the first substeps of a timestamped call record their marks)
        if (st == WGS_OK) {
            const int ts_slot = timestamps && d->timing.events.used < Events::MAX_SUBSTEPS ? d->timing.events.used++ : -1;
            if ((st = begin_substep(d, false, ts_slot)) == WGS_OK && (st = enqueue_sort<D>(d)) == WGS_OK && (st = enqueue_p2g<D>(d, P2gLayers::all)) == WGS_OK)
                st = enqueue_finish<D>(d);
        }
        if (st != WGS_OK) {   // (the substeps enqueued so far stand: a pose read-back after a failed call sees their bodies integrated)
            flush_bodies();
            return st;
        }
    }
    flush_bodies();
    if (timestamps) d->timing.pending = true;
    return watch_counters(d);
}

wgs_status wgs_sync(wgs_data *d) {
    WGS_TRY(enter(d, true, "data is NULL"));
    WGS_TRY(fetch_counters(d));
    return sticky_status(d);
}

}  // extern "C"
