// capi_io.inc — entry points that write simulation inputs and read state back: sim params, colliders, bodies, rigid
// (mesh) particles, plastic state; particles, positions, grid, blocks, body poses, the vertex buffer, device pointers,
// timings and stats. Every reader that needs a staging buffer takes a Scratch and ends in download(); the kernels they
// launch are in kernels_readback.h / kernels_shard.h. In front: the host rules several entry points share (fill_sim_params,
// cdf_live, "this collider moves": colliders_move; the one list of the rigid-particle buffers: rigid_arrays), the stages of
// capi_lifecycle.inc's create_impl among their users.

namespace {
__global__ void k_fluid_collapse(Dev d, int side);   // kernels_fluid.h (defined behind every other kernel: capi.hip on placement)
__global__ void k_models_scatter(Dev d, int side, const uint8_t *by_pid);   // kernels_models.h (likewise)
__global__ void k_models_gather(Dev d, int side, uint8_t *by_pid);
__global__ void k_fluid_collapse_masked(Dev d, int side);

// back to the data's single model: the planes are released once nothing in flight reads them
wgs_status drop_particle_models(wgs_data *d) {
    if (!d->dev.pmodel[0]) return WGS_OK;
    WGS_TRY(enter(d));
    HIP_TRY(hipStreamSynchronize(d->stream));
    d->mem.release_group(MemGroup::models);
    d->dev.pmodel[0] = d->dev.pmodel[1] = nullptr;
    return WGS_OK;
}

void fill_sim_params(SimParamsDev &sp, const wgs_sim_params *params) {
    for (int k = 0; k < D; k++) sp.gravity[k] = params->gravity[k];
    sp.dt = params->dt;
}

// After a step with zero colliders every particle cdf is default_cdf()
// (g2p_cdf.wgsl:246-249 runs unconditionally); before any step the input is echoed.
bool cdf_live(const wgs_data *d) { return d->cpic || d->substeps == 0; }

// "This collider moves", by the two kinds of evidence: a velocity among the first n colliders the host wrote, a mass
// property of any. Both end in colliders_move.
uint32_t moving_by_velocity(const wgs_data *d, size_t n) {
    uint32_t mask = 0u;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++)
            if (d->host_colliders[i].linvel[k] != 0.f || d->host_colliders[i].angvel[k] != 0.f) mask |= 1u << i;
    return mask;
}
uint32_t moving_by_mass(const wgs_data *d) {
    uint32_t mask = 0u;
    for (size_t i = 0; i < d->dev.n_colliders; i++) {
        const BodyDev &b = d->host_bodies[i];
        for (int k = 0; k < 3; k++) if (b.inv_mass[k] != 0.f) mask |= 1u << i;
        for (int k = 0; k < 9; k++) if (b.inv_inertia_local[k] != 0.f) mask |= 1u << i;
    }
    return mask;
}
// (both sticky; says whether the set of moving colliders changed. create_impl stops here: new data has no cached node cdfs,
// and it enables the impulses behind its last launch, under its own error text)
bool note_moving(wgs_data *d, uint32_t mask) {
    const uint32_t moving_before = d->moving_mask;
    d->moving_mask |= mask;
    d->bodies_move = d->bodies_move || mask != 0u;
    return d->moving_mask != moving_before;
}
// The buffers of the mesh colliders' samples (n) and vertices (nv), MemGroup::rigid — listed HERE AND NOWHERE ELSE. Every
// pointer is forgotten first (the caller released the group), so 0, 0 leaves the data without them.
wgs_status rigid_arrays(wgs_data *d, size_t n, size_t nv) {
    Dev &dev = d->dev;
    auto rigid_array = [&](auto **ptr, size_t count) {
        *ptr = nullptr;
        return count ? dev_alloc(d, ptr, count, MemGroup::rigid) : WGS_OK;
    };
    WGS_TRY(rigid_array(&dev.rp_local, n * D));
    WGS_TRY(rigid_array(&dev.rp_world, n * D));
    WGS_TRY(rigid_array(&dev.rp_ids, n));
    WGS_TRY(rigid_array(&dev.rv_local, nv * D));
    WGS_TRY(rigid_array(&dev.rv_world, nv * D));
    WGS_TRY(rigid_array(&dev.rv_collider, nv));
    WGS_TRY(rigid_array(&dev.rp_needs, n));
    return WGS_OK;
}
wgs_status colliders_move(wgs_data *d, uint32_t mask) {
    if (note_moving(d, mask)) d->cdf_generation++;   // (what keeps of a block's node cdfs depends on which colliders move)
    return d->bodies_move ? enable_impulses(d) : WGS_OK;
}
}

extern "C" {

wgs_status wgs_set_uniform_material(wgs_data *d, float mass, float init_volume, float lambda, float mu) {
    WGS_TRY(enter(d, true, "data is NULL"));
    if (D != 3) return WGS_OK;  // the 2D layout has no separate constants quad: nothing to gain
    if (d->substeps != 0) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_uniform_material: call before the first step");
    if (d->dev.uniform) return WGS_OK;
    d->dev.uniform = 1u;
    d->dev.uni_mass = mass;
    d->dev.uni_vol = init_volume;
    d->dev.uni_lambda = lambda;
    d->dev.uni_mu = mu;
    if (d->dev.n) hipLaunchKernelGGL(k_to_uniform, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, 1);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_set_grid_growth(wgs_data *d, int32_t enabled) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    d->auto_grow = enabled != 0;
    return WGS_OK;
}

wgs_status wgs_set_constitutive_model(wgs_data *d, int32_t model) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (model != WGS_MODEL_COROTATED && model != WGS_MODEL_NEO_HOOKEAN && model != WGS_MODEL_FLUID) return fail(WGS_ERR_INVALID_ARGUMENT, "unknown model");
    // (snow is defined on the corotated stress and exists as instantiations of that model only: capi_plasticity.inc)
    if (d->plasticity == WGS_PLASTICITY_SNOW && model != WGS_MODEL_COROTATED)
        return fail(WGS_ERR_UNSUPPORTED, "wgs_set_constitutive_model: WGS_PLASTICITY_SNOW is set (wgs_set_plasticity_model): the corotated model only");
    if (model == WGS_MODEL_FLUID) {
        // (only the instantiations without plastic state exist for the fluid: host_substep.inc launch_g2p)
        if (d->plastic) return fail(WGS_ERR_UNSUPPORTED, "WGS_MODEL_FLUID: this data's step carries plastic state (Drucker-Prager particles, phases or force_plastic)");
    }
    WGS_TRY(drop_particle_models(d));   // (one model for all particles again: wgs_set_particle_models)
    if (model == WGS_MODEL_FLUID) {
        // the F quads of the current buffer -> diag(det F, 1[, 1]), stream-ordered (kernels_fluid.h; the identity on values already in that
        // form). Switching away needs nothing: diag(J, 1, 1) is a deformation gradient of that volume ratio.
        WGS_TRY(enter(d));
        if (d->dev.n) hipLaunchKernelGGL(k_fluid_collapse, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side);
        HIP_TRY(hipGetLastError());
    }
    d->dev.model = model;
    return WGS_OK;
}

wgs_status wgs_set_particle_models(wgs_data *d, const uint8_t *models) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_particle_models: sharded data (the migration record carries no model): single-domain data only");
    if (!models) return drop_particle_models(d);
    // (only the instantiation without plastic state exists: host_substep.inc launch_g2p)
    if (d->plastic) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_particle_models: this data's step carries plastic state (Drucker-Prager particles, phases or force_plastic)");
    const size_t n = d->dev.n;
    for (size_t i = 0; i < n; i++)
        if (models[i] > WGS_MODEL_FLUID)
            return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_particle_models: entry " + std::to_string(i) + " is " + std::to_string((int)models[i]) + ", not a WGS_MODEL_* (0, 1, 2)");
    WGS_TRY(enter(d));
    Dev &dev = d->dev;
    if (!dev.pmodel[0]) {   // one byte per slot and side, like the pid plane: both planes or neither
        if (dev_alloc(d, &dev.pmodel[0], (size_t)dev.npad, MemGroup::models) != WGS_OK ||
            dev_alloc(d, &dev.pmodel[1], (size_t)dev.npad, MemGroup::models) != WGS_OK) {
            d->mem.release_group(MemGroup::models);
            dev.pmodel[0] = dev.pmodel[1] = nullptr;
            return fail(WGS_ERR_HIP, "wgs_set_particle_models: out of device memory for the model planes");
        }
    }
    if (n) {
        Scratch<uint8_t> tmp;
        WGS_TRY(tmp.alloc(n));
        HIP_TRY(hipMemcpyAsync(tmp.ptr, models, n, hipMemcpyHostToDevice, d->stream));
        hipLaunchKernelGGL(k_models_scatter, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, dev, d->side, tmp.ptr);
        // the fluid's particles -> diag(det F, 1[, 1]), as wgs_set_constitutive_model(WGS_MODEL_FLUID) does for all of them
        hipLaunchKernelGGL(k_fluid_collapse_masked, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, dev, d->side);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(d->stream));
    }
    return WGS_OK;
}

wgs_status wgs_read_particle_models(wgs_data *d, uint8_t *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_read_particle_models: sharded data has one model (wgs_set_constitutive_model)");
    const size_t n = d->dev.n;
    if (n == 0) return WGS_OK;
    Scratch<uint8_t> tmp;
    WGS_TRY(tmp.alloc(n));
    hipLaunchKernelGGL(k_models_gather, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, tmp.ptr);
    HIP_TRY(hipGetLastError());
    return download(d, out, tmp.ptr, n);
}

wgs_status wgs_set_fluid_eos(wgs_data *d, float gamma) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (!(gamma > 1.0f) || !std::isfinite(gamma)) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_fluid_eos: gamma must be finite and > 1");
    d->dev.fluid_gamma = gamma;   // (a kernel argument: the substeps enqueued from here on see it)
    return WGS_OK;
}

wgs_status wgs_set_sim_params(wgs_data *d, const wgs_sim_params *params) {
    WGS_TRY(enter(d, params != nullptr));
    fill_sim_params(d->host_sp, params);
    // pageable memcpyAsync returns after staging, so host_sp may be reused at once
    HIP_TRY(hipMemcpyAsync(d->sp, &d->host_sp, sizeof(SimParamsDev), hipMemcpyHostToDevice, d->stream));
    return WGS_OK;
}

// The setters write single fields of the device-side ColliderDev records (strided copies): poses and
// velocities are integrated on the device, so a whole-record upload would roll them back.
namespace {
wgs_status upload_collider_field(wgs_data *d, size_t field_offset, size_t field_bytes, size_t n) {
    if (n == 0) return WGS_OK;
    HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<char *>(d->colliders) + field_offset, sizeof(ColliderDev),
                             reinterpret_cast<const char *>(d->host_colliders.data()) + field_offset, sizeof(ColliderDev),
                             field_bytes, n, hipMemcpyHostToDevice, d->stream));
    return WGS_OK;
}
}  // namespace

wgs_status wgs_set_collider_poses(wgs_data *d, const wgs_pose *poses, const float *coms, size_t n) {
    WGS_TRY(enter(d, poses || !n));
    if (n > d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "more poses than colliders");
    for (size_t i = 0; i < n; i++) {
        ColliderDev &c = d->host_colliders[i];
        for (int k = 0; k < 4; k++) c.rot[k] = poses[i].rotation[k];
        for (int k = 0; k < 3; k++) c.trans[k] = poses[i].translation[k];
        c.scale = poses[i].scale;
        if (coms) for (int k = 0; k < 3; k++) c.com[k] = coms[i * 3 + k];
    }
    d->cdf_generation++;   // cached node cdfs / block classes are those of the old poses
    static_assert(offsetof(ColliderDev, scale) + sizeof(float) - offsetof(ColliderDev, rot) == 32, "rot|trans|scale contiguous");
    WGS_TRY(upload_collider_field(d, offsetof(ColliderDev, rot), 32, n));
    if (coms) WGS_TRY(upload_collider_field(d, offsetof(ColliderDev, com), sizeof(float) * 3, n));
    // update_world_mass_properties (rigid_impulses.wgsl:138-149) for the new poses; with explicit world
    // centres of mass the local ones are re-derived instead
    if (n) hipLaunchKernelGGL(k_bodies_refresh<D>, dim3(1), dim3(16), 0, d->stream, d->dev, coms ? (uint32_t)((1u << n) - 1u) : 0u);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_set_body_velocities(wgs_data *d, const wgs_velocity *vels, size_t n) {
    WGS_TRY(enter(d, vels || !n));
    if (n > d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "more velocities than colliders");
    for (size_t i = 0; i < n; i++) {
        ColliderDev &c = d->host_colliders[i];
        for (int k = 0; k < 3; k++) c.linvel[k] = vels[i].linear[k];
        for (int k = 0; k < 3; k++) c.angvel[k] = vels[i].angular[k];
    }
    WGS_TRY(colliders_move(d, moving_by_velocity(d, n)));
    static_assert(offsetof(ColliderDev, angvel) - offsetof(ColliderDev, linvel) == 12, "linvel|angvel contiguous");
    return upload_collider_field(d, offsetof(ColliderDev, linvel), sizeof(float) * 6, n);
}

wgs_status wgs_set_body_mass_properties(wgs_data *d, const wgs_mass_properties *mp, size_t n) {
    WGS_TRY(enter(d, mp || !n));
    if (n > d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "more mass properties than colliders");
    for (size_t i = 0; i < n; i++) {
        BodyDev &b = d->host_bodies[i];
        for (int k = 0; k < 3; k++) b.inv_mass[k] = mp[i].inv_mass[k];
        for (int k = 0; k < 9; k++) b.inv_inertia_local[k] = mp[i].inv_inertia_local[k];
    }
    WGS_TRY(colliders_move(d, moving_by_mass(d)));
    // inv_mass | inv_inertia_local are the first 12 floats of BodyDev; local_com / world inertia stay device-owned
    static_assert(offsetof(BodyDev, local_com) == sizeof(float) * 12, "BodyDev layout");
    if (n)
        HIP_TRY(hipMemcpy2DAsync(d->dev.bodies, sizeof(BodyDev), d->host_bodies.data(), sizeof(BodyDev), sizeof(float) * 12, n,
                                 hipMemcpyHostToDevice, d->stream));
    if (n) hipLaunchKernelGGL(k_bodies_refresh<D>, dim3(1), dim3(16), 0, d->stream, d->dev, 0u);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_set_rigid_particles(wgs_data *d, const float *local_points, const wgs_sample_ids *ids, size_t n,
                                   const float *local_vertices, const uint32_t *vertex_collider_ids, size_t nv) {
    WGS_TRY(enter(d));
    if (n && (!local_points || !ids || !local_vertices || !vertex_collider_ids || !nv))
        return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    // (sharded data: every rank holds every sample — the node cdfs are a function of position and colliders, both ranks of a
    // face compute the same values for the nodes they share, nothing about them is exchanged)
    if (n > 0xffffffffull || nv > 0xffffffffull) return fail(WGS_ERR_INVALID_ARGUMENT, "too many samples");
    for (size_t i = 0; i < n; i++) {
        if (ids[i].collider >= d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "sample of an unknown collider");
        for (int k = 0; k < D; k++)
            if (ids[i].vertex[k] >= nv) return fail(WGS_ERR_INVALID_ARGUMENT, "sample refers to a vertex out of range");
    }
    for (size_t i = 0; i < nv; i++)
        if (vertex_collider_ids[i] >= d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "vertex of an unknown collider");
    HIP_TRY(hipStreamSynchronize(d->stream));
    Dev &dev = d->dev;
    dev.n_rigid = 0;
    // buffers of an earlier call are released (the mesh accumulators, sized by the grid capacity, are kept)
    d->mem.release_group(MemGroup::rigid);
    WGS_TRY(rigid_arrays(d, 0, 0));
    if (n == 0) return WGS_OK;
    WGS_TRY(rigid_arrays(d, n, nv));
    d->mesh_cdf = true;   // (the mesh accumulators belong to the grid group: alloc_grid lists them)
    WGS_TRY(alloc_grid(d, true));
    std::vector<uint4> packed(n);
    for (size_t i = 0; i < n; i++)
        packed[i] = make_uint4(ids[i].vertex[0], ids[i].vertex[1], D == 3 ? ids[i].vertex[2] : 0u, ids[i].collider);
    HIP_TRY(hipMemcpyAsync(dev.rp_local, local_points, sizeof(float) * n * D, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(dev.rp_ids, packed.data(), sizeof(uint4) * n, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(dev.rv_local, local_vertices, sizeof(float) * nv * D, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipMemcpyAsync(dev.rv_collider, vertex_collider_ids, sizeof(uint32_t) * nv, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    dev.n_rigid = (uint32_t)n;
    dev.n_rvtx = (uint32_t)nv;
    return WGS_OK;
}

wgs_status wgs_read_body_poses(wgs_data *d, wgs_pose *poses, wgs_velocity *vels, float *coms, size_t n) {
    WGS_TRY(enter(d, poses || !n));
    if (n > d->dev.n_colliders) return fail(WGS_ERR_INVALID_ARGUMENT, "more poses than colliders");
    std::vector<ColliderDev> tmp(WGS_MAX_COLLIDERS);
    WGS_TRY(download(d, tmp.data(), d->colliders, sizeof(ColliderDev) * WGS_MAX_COLLIDERS));
    for (size_t i = 0; i < n; i++) {
        const ColliderDev &c = tmp[i];
        for (int k = 0; k < 4; k++) poses[i].rotation[k] = c.rot[k];
        for (int k = 0; k < 3; k++) poses[i].translation[k] = c.trans[k];
        poses[i].scale = c.scale;
        if (vels) {
            for (int k = 0; k < 3; k++) vels[i].linear[k] = c.linvel[k];
            for (int k = 0; k < 3; k++) vels[i].angular[k] = c.angvel[k];
        }
        if (coms) for (int k = 0; k < 3; k++) coms[i * 3 + k] = c.com[k];
    }
    return WGS_OK;
}

wgs_status wgs_read_positions(wgs_data *d, float *out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "sharded wgs_data: use wgs_shard_export");
    if (d->dev.n == 0) return WGS_OK;
    Scratch<float> tmp;
    WGS_TRY(tmp.alloc((size_t)D * d->dev.n));
    hipLaunchKernelGGL(k_export_positions, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, tmp.ptr);
    return download(d, out, tmp.ptr, sizeof(float) * D * (size_t)d->dev.n);
}

wgs_status wgs_get_device_ptrs(wgs_data *d, wgs_device_ptrs *out) {
    if (!d || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "sharded wgs_data: use wgs_shard_export");
    const float *buf = d->dev.buf[d->side];
    out->position_quads = buf + (size_t)Pl<D>::XM * 4 * d->dev.npad;
    out->particle_ids = pid_plane<D>(buf, d->dev.npad);
    out->count = d->dev.n;
    out->capacity = d->dev.npad;
    out->dim = D;
    out->reserved = 0;
    out->hip_stream = d->stream;
    return WGS_OK;
}

wgs_status wgs_read_particles(wgs_data *d, wgs_particle *out, wgs_plastic_state *plastic_out) {
    WGS_TRY(enter(d, out != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "sharded wgs_data: use wgs_shard_export");
    const uint32_t n = d->dev.n;
    if (n == 0) return WGS_OK;
    static_assert(sizeof(wgs_particle) % 4 == 0, "wgs_particle must be word-sized");
    ParticleOffsets o;
#define OFF(f) (uint32_t)(offsetof(wgs_particle, f) / 4)
    o.stride = sizeof(wgs_particle) / 4;
    o.pos = OFF(position); o.vel = OFF(dynamics.velocity); o.F = OFF(dynamics.def_grad); o.C = OFF(dynamics.affine);
    o.nrm = OFF(dynamics.cdf.normal); o.rvel = OFF(dynamics.cdf.rigid_vel); o.dist = OFF(dynamics.cdf.signed_distance);
    o.aff = OFF(dynamics.cdf.affinity); o.vol = OFF(dynamics.init_volume); o.rad = OFF(dynamics.init_radius);
    o.mass = OFF(dynamics.mass); o.lam = OFF(model.lambda); o.mu = OFF(model.mu); o.has_pl = OFF(has_plasticity);
    o.dp = OFF(plasticity); o.has_ph = OFF(has_phase); o.phase = OFF(phase);
#undef OFF
    Scratch<wgs_particle> tmp;
    Scratch<float> ptmp;   // (stays null unless asked for: the kernel then skips it)
    WGS_TRY(tmp.alloc(n));
    if (plastic_out) WGS_TRY(ptmp.alloc((size_t)3 * n));
    hipLaunchKernelGGL(k_export_particles, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, o, d->plastic,
                       cdf_live(d), (uint32_t)d->substeps, d->static_radius, d->static_dp, d->static_phase, d->static_flags,
                       reinterpret_cast<float *>(tmp.ptr), ptmp.ptr);
    if (plastic_out) HIP_TRY(hipMemcpyAsync(plastic_out, ptmp.ptr, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, d->stream));
    return download(d, out, tmp.ptr, sizeof(wgs_particle) * (size_t)n);   // (one wait for both copies)
}

wgs_status wgs_prep_vertex_buffer_device(wgs_data *d, uint32_t mode, wgs_instance *device_instances) {
    WGS_TRY(enter(d, device_instances != nullptr));
    if (mode > WGS_RENDER_CDF_SIGNS) return fail(WGS_ERR_INVALID_ARGUMENT, "unknown render mode");
    if (d->dev.n)
        hipLaunchKernelGGL(k_prep_instances, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, mode, cdf_live(d),
                           (uint32_t)d->substeps, reinterpret_cast<float *>(device_instances));
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

wgs_status wgs_prep_vertex_buffer(wgs_data *d, uint32_t mode, wgs_instance *instances) {
    WGS_TRY(enter(d, instances != nullptr));
    if (mode > WGS_RENDER_CDF_SIGNS) return fail(WGS_ERR_INVALID_ARGUMENT, "unknown render mode");
    const size_t bytes = sizeof(wgs_instance) * (size_t)d->dev.n;
    if (bytes == 0) return WGS_OK;
    Scratch<wgs_instance> tmp;
    WGS_TRY(tmp.alloc(d->dev.n));
    HIP_TRY(hipMemcpyAsync(tmp.ptr, instances, bytes, hipMemcpyHostToDevice, d->stream));  // base colours
    WGS_TRY(wgs_prep_vertex_buffer_device(d, mode, tmp.ptr));
    return download(d, instances, tmp.ptr, bytes);
}

wgs_status wgs_set_plastic_state(wgs_data *d, const wgs_plastic_state *states) {
    WGS_TRY(enter(d, states != nullptr));
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "plastic-state restore addresses particles by local index: single-domain data only");
    const size_t n = d->dev.n;
    if (n == 0 || !d->plastic) return WGS_OK;  // no particle carries plasticity: nothing reads the state
    Scratch<float> tmp;
    WGS_TRY(tmp.alloc(3 * n));
    HIP_TRY(hipMemcpyAsync(tmp.ptr, states, sizeof(float) * 3 * n, hipMemcpyHostToDevice, d->stream));
    hipLaunchKernelGGL(k_import_plastic_state, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, tmp.ptr);
    HIP_TRY(hipStreamSynchronize(d->stream));
    return WGS_OK;
}

wgs_status wgs_read_grid(wgs_data *d, wgs_node_record *out, size_t capacity, size_t *count) {
    WGS_TRY(enter(d, count != nullptr));
    WGS_TRY(fetch_counters(d));
    const size_t total = (size_t)d->seen.sync_nblocks * NPB;
    *count = total;
    if (!out || total == 0) return WGS_OK;
    if (capacity < total) return fail(WGS_ERR_INVALID_ARGUMENT, "capacity too small; *count holds the required size");
    Scratch<wgs_node_record> tmp;
    WGS_TRY(tmp.alloc(total));
    hipLaunchKernelGGL(k_export_grid, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->seen.sync_nblocks, d->cpic, tmp.ptr);
    return download(d, out, tmp.ptr, sizeof(wgs_node_record) * total);
}

wgs_status wgs_read_blocks(wgs_data *d, wgs_block_record *out, size_t capacity, size_t *count, uint32_t *sorted_ids) {
    WGS_TRY(enter(d, count != nullptr));
    WGS_TRY(fetch_counters(d));
    const size_t total = d->seen.sync_nblocks;
    *count = total;
    if (out && total) {
        if (capacity < total) return fail(WGS_ERR_INVALID_ARGUMENT, "capacity too small; *count holds the required size");
        Scratch<wgs_block_record> tmp;
        WGS_TRY(tmp.alloc(total));
        hipLaunchKernelGGL(k_export_blocks, dim3(grid_for(d, 1)), dim3(256), 0, d->stream, d->dev, d->seen.sync_nblocks, tmp.ptr);
        WGS_TRY(download(d, out, tmp.ptr, sizeof(wgs_block_record) * total));
    }
    if (sorted_ids && d->dev.n) {
        // The buffer written by the last substep is in sorted order: its pid plane IS sorted_ids.
        WGS_TRY(download(d, sorted_ids, pid_plane<D>(d->dev.buf[d->side], d->dev.npad), sizeof(uint32_t) * (size_t)d->dev.n));
    }
    return WGS_OK;
}

// a slab's particles as exchange records, into device memory of the caller (kernels_shard.h)
wgs_status wgs_shard_export(wgs_data *d, void *device_buf, uint32_t capacity_records, uint32_t *count) {
    WGS_TRY(enter(d, device_buf && count));
    if (!d->dev.sharded) return fail(WGS_ERR_INVALID_ARGUMENT, "not a sharded wgs_data");
    catch_up_counters(d);
    hipLaunchKernelGGL(k_clear_headers, dim3(1), dim3(64), 0, d->stream, static_cast<uint32_t *>(device_buf), (uint32_t *)nullptr);
    hipLaunchKernelGGL(k_export_records<D>, dim3(grid_for(d, 4)), dim3(256), 0, d->stream, d->dev, d->side, static_cast<float *>(device_buf), capacity_records);
    WGS_TRY(download(d, count, device_buf, sizeof(uint32_t)));
    if (*count > capacity_records) return fail(WGS_ERR_INVALID_ARGUMENT, "export buffer too small");
    return WGS_OK;
}

wgs_status wgs_read_timing_overhead(wgs_data *d, float *ms_per_mark) {
    WGS_TRY(enter(d, ms_per_mark != nullptr));
    resolve_timings(d);
    *ms_per_mark = d->timing.mark_overhead_ms;
    return WGS_OK;
}

wgs_status wgs_read_timings(wgs_data *d, float ms[WGS_NUM_PASSES]) {
    WGS_TRY(enter(d, ms != nullptr));
    resolve_timings(d);
    for (int p = 0; p < WGS_NUM_PASSES; p++) ms[p] = d->timing.ms[p];
    return WGS_OK;
}

wgs_status wgs_get_stats(wgs_data *d, wgs_stats *out) {
    WGS_TRY(enter(d, out != nullptr));
    WGS_TRY(fetch_counters(d));
    out->num_particles = d->dev.n;
    if (d->dev.sharded) {
        WGS_TRY(download(d, &out->num_particles, d->dev.counters + CTR_NV + CTR_SET * (d->sub.needs_compact ? ((d->substeps & 1) ^ 1) : (d->substeps & 1)), sizeof(uint32_t)));
    }
    out->num_active_blocks = d->seen.sync_nblocks;
    out->grid_capacity = d->dev.cap;
    out->overflow = d->seen.errors;
    out->substeps_done = d->substeps;
    out->device_bytes = d->mem.bytes();
    out->num_near_collider_blocks = d->cpic && d->seen.ncpic != UINT32_MAX ? d->seen.ncpic : 0u;
    out->grid_growths = d->stats.grid_grown;
    out->cell_changers = d->stats.movers_total;
    out->table_rebuilds = d->stats.table_rebuilds;
    out->block_ids = d->seen.nphys;
    out->block_ids_free = d->seen.nfree;
    out->table_marks = d->seen.ntomb;
    out->table_refreshes = (uint32_t)d->stats.table_refreshes;
    return WGS_OK;
}

}  // extern "C"
