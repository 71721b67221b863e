// capi_lifecycle.inc — entry points that make, advance and end a simulation: library info, pipeline and data create /
// destroy, wgs_set_stream, wgs_step, wgs_sync. In front: the stages of data creation, in the order create_impl runs them
// (check_create_args, init_scalars, alloc_particle_state, stage_particles with pack_slot, the two uniform detections, the
// uploads, the colliders, the conversion to the uniform layouts).

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

// What wgs_data_create / wgs_data_create_sharded were asked for.
struct CreateSpec {
    wgs_pipeline *pipeline;
    const wgs_sim_params *params;
    const wgs_particle *particles;
    size_t n;
    const uint32_t *global_ids;   // null: a particle's id is its index
    const wgs_collider *colliders;
    size_t num_colliders;
    float cell_width;
    uint32_t grid_capacity;
    size_t particle_capacity;     // (raised to n by check_create_args)
    bool sharded;
    int32_t block_lo, block_hi, force_plastic;
};

wgs_status check_create_args(CreateSpec &c, wgs_data **out) {
    if (!c.pipeline || !c.params || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (c.n && !c.particles) return fail(WGS_ERR_INVALID_ARGUMENT, "particles is NULL");
    if (c.num_colliders && !c.colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "colliders is NULL");
    if (c.num_colliders > WGS_MAX_COLLIDERS)
        return fail(WGS_ERR_UNSUPPORTED, "at most 16 coupled colliders (grid.wgsl:230-240)");
    if (!(c.cell_width > 0.f)) return fail(WGS_ERR_INVALID_ARGUMENT, "cell_width must be > 0");
    if (c.grid_capacity == 0 || c.grid_capacity > (1u << 25)) return fail(WGS_ERR_INVALID_ARGUMENT, "grid_capacity out of range");
    // 32-bit byte offsets inside one ping-pong buffer (layout.h ldp/stp)
    if (c.particle_capacity < c.n) c.particle_capacity = c.n;
    if (buffer_floats<D>((uint32_t)c.particle_capacity + 64) * 4 >= (1ull << 32))
        return fail(WGS_ERR_UNSUPPORTED, "more than ~21M particles per wgs_data: shard across GPUs");
    return WGS_OK;
}

// The scalar fields of Dev and of the handle, and the environment switches, read once, here.
void init_scalars(wgs_data *d, const CreateSpec &c) {
    Dev &dev = d->dev;
    dev.n = dev.nv = (uint32_t)c.n;
    dev.sharded = c.sharded ? 1u : 0u;
    dev.shard_lo = c.sharded ? c.block_lo : INT32_MIN;
    dev.shard_hi = c.sharded ? c.block_hi : INT32_MAX;
    d->capacity = (uint32_t)c.particle_capacity;
    dev.npad = (((uint32_t)c.particle_capacity + 63u) / 64u) * 64u;
    if (dev.npad == 0) dev.npad = 64;
    dev.cap = next_pow2(c.grid_capacity);  // grid.rs:283
    dev.hmask = dev.cap * 2u - 1u;  // half-full table (reference: exactly cap slots, quirk B4)
    dev.h = c.cell_width;
    dev.inv_h = 1.0f / c.cell_width;
    {
        int e = 0;
        dev.h_pow2 = (frexpf(c.cell_width, &e) == 0.5f) ? 1u : 0u;
    }
    dev.model = WGS_MODEL_COROTATED;
    dev.fluid_gamma = 7.0f;   // (wgs_set_fluid_eos)
    // developer switches (layout.h DebugSwitch); 0 in production
    dev.dbg = getenv("WGS_DEBUG") ? (uint32_t)strtoul(getenv("WGS_DEBUG"), nullptr, 0) : 0u;
#ifndef WGS_ABLATE
    dev.dbg &= WGS_LAUNCH_SHAPE_SWITCHES;
#endif
    // data that evicts its long-inactive blocks (alloc_grid gives it a free list under the same switch) needs no periodic table
    // rebuild: the marks the evictions leave are cleared by k_table_refresh, without touching a particle — slabs of a
    // decomposition included since round 6
    if (getenv("WGS_REHASH_PERIOD")) d->rehash_period = std::max(1u, (uint32_t)strtoul(getenv("WGS_REHASH_PERIOD"), nullptr, 0));  // same results
    else if (!(dev.dbg & DBG_NO_EVICTION)) d->rehash_period = 0u;
    dev.n_colliders = (uint32_t)c.num_colliders;
    d->cpic = c.num_colliders > 0;
}

// (the order of the allocations decides addresses, and addresses decide channel placement: keep it)
wgs_status alloc_particle_state(wgs_data *d, const CreateSpec &c) {
    Dev &dev = d->dev;
    WGS_TRY(dev_alloc(d, &dev.buf[0], buffer_floats<D>(dev.npad)));
    WGS_TRY(dev_alloc(d, &dev.buf[1], buffer_floats<D>(dev.npad)));
    WGS_TRY(dev_alloc(d, &dev.perm, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.perm_cell, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.cellid, (size_t)dev.npad));
    WGS_TRY(dev_alloc(d, &dev.mv_next, (size_t)dev.npad));
    WGS_TRY(alloc_grid(d));
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
    if (c.sharded) {
        dev.leavers_cap = std::max<uint32_t>(4096u, (uint32_t)(c.particle_capacity / 16));
        WGS_TRY(dev_alloc(d, &dev.leavers, (size_t)dev.leavers_cap));
    }
    dev.sp = d->sp;
    dev.colliders = d->colliders;
    return WGS_OK;
}

// quad q of slot i in the host image of a buffer (floats: it sits at float (q * npad + i) * 4)
float *slot_quad(float *image, uint32_t npad, int q, uint32_t i) { return image + ((size_t)q * npad + i) * 4; }

// One particle into slot i of the image: the host inverse of unpack_slot (kernels_readback.h), quad by quad in the words of
// layout.h's table. `dp`: its six Drucker-Prager parameters or the defaults; the plastic state starts as
// DruckerPragerPlasticState::default() = {1, 1, 0}, drucker_prager.rs:44-53.
template <int DIM>
void pack_slot(float *image, uint32_t npad, uint32_t i, const wgs_particle &q, const float *dp, float phase, float max_stretch) {
    using L = Pl<DIM>;
    const wgs_particle_dynamics &dy = q.dynamics;
    const float *x = q.position, *v = dy.velocity, *F = dy.def_grad, *C = dy.affine, *nrm = dy.cdf.normal, *rvel = dy.cdf.rigid_vel;
    const float lambda = q.model.lambda, mu = q.model.mu, dist = dy.cdf.signed_distance;
    float aff;
    memcpy(&aff, &dy.cdf.affinity, 4);
    auto put = [&](int quad, float a, float b, float c, float d) {
        float *p = slot_quad(image, npad, quad, i);
        p[0] = a; p[1] = b; p[2] = c; p[3] = d;
    };
    if constexpr (DIM == 3) {
        put(L::XM, x[0], x[1], x[2], dy.mass);
        put(L::CV0, C[0], C[1], C[2], C[3]);
        put(L::CV1, C[4], C[5], C[6], C[7]);
        put(L::CV2, C[8], v[0], v[1], v[2]);
        put(L::F0, F[0], F[1], F[2], F[3]);
        put(L::F1, F[4], F[5], F[6], F[7]);
        put(L::F2, F[8], dy.init_volume, lambda, mu);
        put(L::CDF0, nrm[0], nrm[1], nrm[2], dist);
        put(L::CDF1, rvel[0], rvel[1], rvel[2], aff);
    } else {
        put(L::XM, x[0], x[1], dy.mass, dy.init_volume);
        put(L::CV0, C[0], C[1], C[2], C[3]);
        put(L::CV2, v[0], v[1], lambda, mu);
        put(L::F0, F[0], F[1], F[2], F[3]);
        put(L::CDF0, nrm[0], nrm[1], dist, aff);
        put(L::CDF1, rvel[0], rvel[1], 0.f, 0.f);
    }
    put(L::DP0, dp[0], dp[1], dp[2], dp[3]);
    put(L::DP1, dp[4], dp[5], 1.0f, 1.0f);
    put(L::DP2, 0.0f, phase, max_stretch, 0.f);
}

// What the host stages of the caller's particles: the image of buffer 0, the by-pid static tables, and whether the
// plasticity / fracture branch ever runs.
struct Staged {
    std::vector<float> image;             // every quad and the pid plane
    std::vector<float> radius, dp, phase; // dp: 6 per particle, phase: (phase, max_stretch)
    std::vector<uint32_t> flags;          // bit0 has_plasticity, bit1 has_phase
    bool plastic = false;
};

// DruckerPrager::new(-1, -1): the six parameters of a particle without plasticity
void default_dp_params(float out[6]) {
    const float deg = 3.14159265358979323846f / 180.0f;
    const float default_dp[6] = {35.0f * deg, 9.0f * deg, 0.2f, 10.0f * deg, -1.0f, -1.0f};
    for (int k = 0; k < 6; k++) out[k] = default_dp[k];
}

// Does the plasticity / fracture branch ever run for this particle? `dp`: its six parameters or the defaults.
// (particle_update.wgsl:98-122; max_stretch >= FLT_MAX can never be exceeded by a finite F)
bool particle_is_plastic(const float *dp, float phase, float max_stretch) {
    return (phase == 0.0f && dp[4] != 0.0f) || (phase > 0.0f && max_stretch > 0.0f && max_stretch < FLT_MAX);
}

// AoS -> SoA staging (GpuParticles::from_particles + GpuModels::from_particles, particle3d.rs:192-210, models/mod.rs:20-49).
// (kernels_emit.h pack_particle does the same on the device for the particles that come later)
Staged stage_particles(const CreateSpec &c, uint32_t npad) {
    Staged st;
    st.image.assign(buffer_floats<D>(npad), 0.f);
    st.radius.assign(npad, 0.f);
    st.dp.assign((size_t)npad * 6, 0.f);
    st.phase.assign((size_t)npad * 2, 0.f);
    st.flags.assign(npad, 0u);
    float default_dp[6];
    default_dp_params(default_dp);
    uint32_t *pids = pid_plane<D>(st.image.data(), npad);
    for (uint32_t i = 0; i < (uint32_t)c.n; i++) {
        const wgs_particle &q = c.particles[i];
        const float *dp = q.has_plasticity ? &q.plasticity.h0 : default_dp;
        const float phase = q.has_phase ? q.phase.phase : 0.0f;            // models/mod.rs:33-36
        const float max_stretch = q.has_phase ? q.phase.max_stretch : -1.0f;
        pack_slot<D>(st.image.data(), npad, i, q, dp, phase, max_stretch);
        pids[i] = c.global_ids ? c.global_ids[i] : i;
        for (int k = 0; k < 6; k++) st.dp[(size_t)i * 6 + k] = dp[k];
        st.phase[(size_t)i * 2] = phase;
        st.phase[(size_t)i * 2 + 1] = max_stretch;
        st.radius[i] = q.dynamics.init_radius;
        st.flags[i] = (q.has_plasticity ? 1u : 0u) | (q.has_phase ? 2u : 0u);
        if (particle_is_plastic(dp, phase, max_stretch)) st.plastic = true;
    }
    return st;
}

// uniform plasticity parameters (bitwise; single-domain data, like the automatic uniform-material mode; layout.h Dev::uni_dp):
// 1 = one set of h0..h3, 2 = all six and max_stretch — the per-particle state is then packed into DP1 of the image
void detect_uniform_plasticity(wgs_data *d, const CreateSpec &c, Staged &st) {
    Dev &dev = d->dev;
    const uint32_t n = (uint32_t)c.n;
    if (!d->plastic || n == 0 || c.sharded || (dev.dbg & DBG_NO_UNIFORM)) return;
    bool u4 = true, u6 = true;
    for (uint32_t i = 1; i < n && u4; i++) {
        u4 = memcmp(&st.dp[(size_t)i * 6], &st.dp[0], 4 * sizeof(float)) == 0;
        u6 = u6 && memcmp(&st.dp[(size_t)i * 6 + 4], &st.dp[4], 2 * sizeof(float)) == 0 && memcmp(&st.phase[(size_t)i * 2 + 1], &st.phase[1], sizeof(float)) == 0;
    }
    if (!u4) return;
    dev.uni_dp = u6 ? 2u : 1u;
    for (int k = 0; k < 6; k++) dev.uni_dpv[k] = st.dp[k];
    dev.uni_max_stretch = st.phase[1];
    if (u6)
        for (uint32_t i = 0; i < n; i++) {
            float *q1 = slot_quad(st.image.data(), dev.npad, P::DP1, i);
            const float *q2 = slot_quad(st.image.data(), dev.npad, P::DP2, i);
            q1[0] = q1[2]; q1[1] = q1[3]; q1[2] = q2[0]; q1[3] = q2[1];   // (st0, st1, st2, phase)
        }
}

// one material for all particles (bitwise)? -> uniform-material mode (layout.h). Sharded data: the caller says so
// (wgs_set_uniform_material), a rank cannot know the other ranks' particles.
bool detect_uniform_material(const Dev &dev, const CreateSpec &c) {
    const wgs_particle *particles = c.particles;
    bool uniform = D == 3 && c.n > 0 && !c.sharded && !(dev.dbg & DBG_NO_UNIFORM);
    for (uint32_t i = 1; i < (uint32_t)c.n && uniform; i++)
        uniform = memcmp(&particles[i].dynamics.mass, &particles[0].dynamics.mass, 4) == 0 &&
                  memcmp(&particles[i].dynamics.init_volume, &particles[0].dynamics.init_volume, 4) == 0 &&
                  memcmp(&particles[i].model, &particles[0].model, sizeof(wgs_elastic_coefficients)) == 0;
    return uniform;
}

wgs_status h2d(wgs_data *d, void *dst, const void *src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream) == hipSuccess ? WGS_OK : fail(WGS_ERR_HIP, "hipMemcpy H2D failed");
}

// (asynchronous: `st` and the caller's arrays outlive create_impl's wait for the stream)
wgs_status upload_particles(wgs_data *d, const CreateSpec &c, const Staged &st) {
    Dev &dev = d->dev;
    WGS_TRY(h2d(d, dev.buf[0], st.image.data(), st.image.size() * sizeof(float)));
    WGS_TRY(h2d(d, d->static_radius, st.radius.data(), st.radius.size() * sizeof(float)));
    WGS_TRY(h2d(d, d->static_dp, st.dp.data(), st.dp.size() * sizeof(float)));
    WGS_TRY(h2d(d, d->static_phase, st.phase.data(), st.phase.size() * sizeof(float)));
    WGS_TRY(h2d(d, d->static_flags, st.flags.data(), st.flags.size() * sizeof(uint32_t)));
    d->host_sp = SimParamsDev{};
    fill_sim_params(d->host_sp, c.params);
    WGS_TRY(h2d(d, d->sp, &d->host_sp, sizeof(SimParamsDev)));
    if (c.sharded) {
        // counts live on the device; the host-side n / nv become the launch bound (allocated capacity)
        const uint32_t cnt[2] = {(uint32_t)c.n, (uint32_t)c.n};
        WGS_TRY(h2d(d, dev.counters + CTR_N, cnt, sizeof(cnt)));
        WGS_TRY(h2d(d, dev.counters + CTR_N + CTR_SET, cnt, sizeof(cnt)));   // (both sets: layout.h ctr_cur / ctr_next)
        dev.n = dev.nv = (uint32_t)c.particle_capacity;
        d->seen.nv_hint = (uint32_t)c.n;
    }
    return WGS_OK;
}

wgs_status upload_colliders(wgs_data *d, const CreateSpec &c) {
    d->host_colliders.resize(WGS_MAX_COLLIDERS);
    memset(d->host_colliders.data(), 0, sizeof(ColliderDev) * WGS_MAX_COLLIDERS);
    for (size_t i = 0; i < c.num_colliders; i++) fill_collider(d->host_colliders[i], c.colliders[i]);
    WGS_TRY(h2d(d, d->colliders, d->host_colliders.data(), sizeof(ColliderDev) * WGS_MAX_COLLIDERS));
    d->host_bodies.assign(WGS_MAX_COLLIDERS, BodyDev{});
    note_moving(d, moving_by_velocity(d, c.num_colliders));
    if (c.num_colliders)  // local centres of mass from the world ones (update_world_mass_properties' inverse)
        hipLaunchKernelGGL(k_bodies_refresh<D>, dim3(1), dim3(16), 0, d->stream, d->dev, 0xffffu);
    if (d->bodies_move && enable_impulses(d) != WGS_OK) return fail(WGS_ERR_HIP, "out of device memory for the impulse accumulators");
    return WGS_OK;
}

// the uploaded general layout -> the uniform ones the detections decided on, on the device
wgs_status to_uniform_layouts(wgs_data *d, const CreateSpec &c, bool uniform_material) {
    Dev &dev = d->dev;
    if (uniform_material) {
        dev.uniform = 1u;
        dev.uni_mass = c.particles[0].dynamics.mass;
        dev.uni_vol = c.particles[0].dynamics.init_volume;
        dev.uni_lambda = c.particles[0].model.lambda;
        dev.uni_mu = c.particles[0].model.mu;
        hipLaunchKernelGGL(k_to_uniform, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, dev, 0, 0);
    }
    if (dev.uni_dp != 0u)   // (the other ping-pong buffer's copy of the quads the step leaves alone: layout.h Dev::uni_dp)
        for (int qd : {(int)P::DP0, (int)P::DP2})
            if (hipMemcpyAsync(slot_quad(dev.buf[1], dev.npad, qd, 0), slot_quad(dev.buf[0], dev.npad, qd, 0), (size_t)dev.npad * 16,
                               hipMemcpyDeviceToDevice, d->stream) != hipSuccess)
                return fail(WGS_ERR_HIP, "hipMemcpy D2D failed");
    return WGS_OK;
}

// Decides nothing itself: the stages above, top to bottom. What reaches the stream, in this order: the zero fills of the
// allocations, the uploads, the colliders' kernel, the conversions.
wgs_status create_impl(CreateSpec c, wgs_data **out) {
    WGS_TRY(check_create_args(c, out));
    *out = nullptr;
    HIP_TRY(hipSetDevice(c.pipeline->device));
    // (destroyed on every return but the last one, which hands it to the caller)
    std::unique_ptr<wgs_data, void (*)(wgs_data *)> guard(new wgs_data(), wgs_data_destroy);
    wgs_data *d = guard.get();
    d->pipeline = c.pipeline;
    WGS_TRY(d->stream.create());
    init_scalars(d, c);
    WGS_TRY(alloc_particle_state(d, c));
    Staged st = stage_particles(c, d->dev.npad);
    d->plastic = st.plastic || c.force_plastic != 0;
    detect_uniform_plasticity(d, c, st);
    const bool uniform_material = detect_uniform_material(d->dev, c);
    WGS_TRY(upload_particles(d, c, st));
    WGS_TRY(upload_colliders(d, c));
    WGS_TRY(to_uniform_layouts(d, c, uniform_material));
    if (hipStreamSynchronize(d->stream) != hipSuccess) return fail(WGS_ERR_HIP, "initial upload failed");
    *out = guard.release();
    return WGS_OK;
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
    std::unique_ptr<wgs_pipeline> p(new wgs_pipeline());
    p->device = hip_device;
    const hipError_t pe = hipGetDeviceProperties(&p->props, hip_device);
    if (pe != hipSuccess) return fail(WGS_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(pe));
    p->num_cus = p->props.multiProcessorCount > 0 ? p->props.multiProcessorCount : 256;
    *out = p.release();
    return WGS_OK;
}

void wgs_pipeline_destroy(wgs_pipeline *pipeline) { delete pipeline; }

wgs_status wgs_data_create(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                           size_t num_particles, const wgs_collider *colliders, size_t num_colliders, float cell_width,
                           uint32_t grid_capacity, wgs_data **out) {
    return create_impl({pipeline, params, particles, num_particles, nullptr, colliders, num_colliders, cell_width,
                        grid_capacity, num_particles, false, 0, 0, 0}, out);
}

wgs_status wgs_data_create_sharded(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                                   size_t num_particles, const uint32_t *global_ids, const wgs_collider *colliders,
                                   size_t num_colliders, float cell_width, uint32_t grid_capacity,
                                   uint32_t particle_capacity, int32_t block_lo, int32_t block_hi, int32_t force_plastic,
                                   wgs_data **out) {
    if (block_lo >= block_hi) return fail(WGS_ERR_INVALID_ARGUMENT, "empty shard range");
    return create_impl({pipeline, params, particles, num_particles, global_ids, colliders, num_colliders, cell_width,
                        grid_capacity, particle_capacity, true, block_lo, block_hi, force_plastic}, out);
}

wgs_status wgs_set_stream(wgs_data *d, void *hip_stream) {
    WGS_TRY(enter(d, true, "data is NULL"));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return d->stream.borrow(static_cast<hipStream_t>(hip_stream));
}

void wgs_data_destroy(wgs_data *d) {
    if (!d) return;
    if (d->stream) hipStreamSynchronize(d->stream);
    d->mem.release_all();
    delete d->link;
    // The members end what they own in reverse order of their declaration (host_state.h): the timing marks, the watch's
    // event and its pinned copy, the diagnostics' pinned copy and, last of all, the stream (if it is the data's own).
    delete d;
}

wgs_status wgs_step(wgs_pipeline *pipeline, wgs_data *d, uint32_t num_substeps, int32_t timestamps) {
    WGS_TRY(enter(d, pipeline != nullptr));
    if (timestamps) {
        WGS_TRY(d->timing.events.create());   // (the first timestamped call)
        d->timing.events.used = 0;
        d->timing.emit_marks.clear();
    }
    WGS_TRY(maintain_grid(d));
    {
        // the last substep's integrate_bodies, however the loop ends: every other entry point finds the bodies integrated (the
        // substeps enqueued before a failure stand: a pose read-back after a failed call sees their bodies integrated)
        ScopeExit flush_bodies{[d] {
            if (d->sub.bodies_pending) launch_bodies_integrate(d);
            d->sub.bodies_pending = false;
        }};
        for (uint32_t i = 0; i < num_substeps; i++) {
            if (i > 0 && i % 64u == 0u) {  // long calls: keep an eye on the table inside the call too (bounded run-ahead)
                WGS_TRY(watch_counters(d));
                WGS_TRY(maintain_grid(d));
            }
            // (a whole substep: the four stages of host_substep.inc; the first substeps of a timestamped call record their marks)
            const int ts_slot = timestamps && d->timing.events.used < Events::MAX_SUBSTEPS ? d->timing.events.used++ : -1;
            // (the emitters whose batch is due in front of this substep: new slots behind the residents, and the substep rebuilds the table)
            // (ahead of them the sinks that are due: the room they free is the emitters' — the one place a substep may wait for the stream)
            if (d->sinks_set) WGS_TRY(fire_sinks(d, ts_slot >= 0));
            if (d->emit_set) WGS_TRY(fire_emitters(d, ts_slot >= 0));
            WGS_TRY(begin_substep(d, false, ts_slot));
            WGS_TRY(enqueue_sort<D>(d));
            WGS_TRY(enqueue_p2g<D>(d, P2gLayers::all));
            WGS_TRY(enqueue_finish<D>(d));
        }
    }
    if (timestamps) d->timing.pending = true;
    return watch_counters(d);
}

wgs_status wgs_sync(wgs_data *d) {
    WGS_TRY(enter(d, true, "data is NULL"));
    WGS_TRY(fetch_counters(d));
    return sticky_status(d);
}

}  // extern "C"
