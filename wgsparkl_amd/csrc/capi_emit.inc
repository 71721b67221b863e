// capi_emit.inc — particles added at run time (include/wgsparkl_hip_emit.h): the host side of kernels_emit.h. What a record must be for
// the data's layout to hold it (layout_problem), the launch both paths share (PackArgs, grew_by), fire_emitters — which wgs_step asks
// in front of every substep of data that has emitters (declared in host_substep.inc) — and the entry points. The new slots stand
// behind the residents of the current buffer; dev.n / dev.nv — host values on single-domain data — are raised, and the next substep
// rebuilds the block table (seen.force_rehash), whose full binning pass takes the buffer in any order.

namespace {

// empty: the data's layout holds the record; else the mismatch, in words
std::string layout_problem(const wgs_data *d, const wgs_particle &q, bool labelled_fluid) {
    const Dev &dev = d->dev;
    float default_dp[6];
    default_dp_params(default_dp);
    const float *dp = q.has_plasticity ? &q.plasticity.h0 : default_dp;
    const float phase = q.has_phase ? q.phase.phase : 0.0f, max_stretch = q.has_phase ? q.phase.max_stretch : -1.0f;
    if (!d->plastic && particle_is_plastic(dp, phase, max_stretch))
        return "it carries plasticity or a phase that fractures, and this data's step carries no plastic state (create the data with such a particle)";
    if (d->plastic && labelled_fluid) return "it is labelled WGS_MODEL_FLUID, and this data's step carries plastic state";
    if (dev.uniform && (memcmp(&q.dynamics.mass, &dev.uni_mass, 4) != 0 || memcmp(&q.dynamics.init_volume, &dev.uni_vol, 4) != 0 ||
                        memcmp(&q.model.lambda, &dev.uni_lambda, 4) != 0 || memcmp(&q.model.mu, &dev.uni_mu, 4) != 0))
        return "its (mass, init_volume, lambda, mu) differ from the uniform-material constants this data was created under";
    if (dev.uni_dp != 0u && memcmp(dp, dev.uni_dpv, 4 * sizeof(float)) != 0)
        return "its plasticity parameters h0..h3 differ from the uniform ones this data was created under";
    if (dev.uni_dp == 2u && (memcmp(dp + 4, dev.uni_dpv + 4, 2 * sizeof(float)) != 0 || memcmp(&max_stretch, &dev.uni_max_stretch, 4) != 0))
        return "its plasticity lambda, mu or max_stretch differ from the uniform ones this data was created under";
    return std::string();
}

PackArgs pack_args(const wgs_data *d) {
    PackArgs a{};
    a.side = d->side;
    a.stamp = (uint32_t)d->substeps;
    default_dp_params(a.default_dp);
    a.s_radius = d->static_radius;
    a.s_dp = d->static_dp;
    a.s_phase = d->static_phase;
    a.s_flags = d->static_flags;
    return a;
}

// `k` slots behind the residents now hold particles: the counts every launch gets, and what the next substep must not assume
void grew_by(wgs_data *d, uint32_t k) {
    d->dev.n += k;
    d->dev.nv = d->dev.n;
    d->seen.force_rehash = true;    // the next substep bins the whole buffer through the table (k_bin), in whatever order it stands
    d->sub.prev_sorted = false;     // ... which is no longer the sorted output of the last substep (begin_substep drops what its G2P pre-binned)
}

uint64_t batch_size(const wgs_emitter &e) {
    uint64_t total = 1;
    for (int k = 0; k < D; k++) total *= e.count[k];   // (each below 2^32: the product of three may wrap only beyond any capacity, checked per factor)
    return total;
}

// nullptr: acceptable; else what is wrong with it (layout mismatches apart: layout_problem)
const char *emitter_problem(const wgs_data *d, const wgs_emitter &e) {
    if (e.model > WGS_MODEL_FLUID) return "wgs_set_emitters: model must be a WGS_MODEL_* (0, 1, 2)";
    if (e.period == 0u) return "wgs_set_emitters: period must be >= 1";
    uint64_t total = 1;
    for (int k = 0; k < D; k++) {
        if (e.count[k] == 0u) return "wgs_set_emitters: every count must be >= 1";
        if (e.count[k] > d->capacity) return "wgs_set_emitters: one batch is larger than the particle capacity";
        total *= e.count[k];
        if (total > d->capacity) return "wgs_set_emitters: one batch is larger than the particle capacity";
    }
    if (!std::isfinite(e.jitter) || e.jitter < 0.f || e.jitter > 0.5f) return "wgs_set_emitters: jitter must be in [0, 0.5]";
    if (!std::isfinite(e.spacing)) return "wgs_set_emitters: spacing must be finite";
    return nullptr;
}

// The batches that are due in front of the substep about to be enqueued (the schedule of include/wgsparkl_hip_emit.h): one launch per
// firing emitter, the emitter as a by-value argument. Host integers only; nothing waits for the device.
wgs_status fire_emitters(wgs_data *d, bool timed) {
    const uint64_t s = d->substeps;
    bool fired = false;
    for (uint32_t e = 0; e < d->emit_n; e++) {
        const wgs_emitter &em = d->emitters[e];
        if (s < em.start_substep || (s - em.start_substep) % em.period != 0u) continue;
        const uint64_t q = (s - em.start_substep) / em.period;
        if (em.batches != 0u && q >= em.batches) continue;
        const uint64_t total = batch_size(em);
        if ((uint64_t)d->dev.n + total > d->capacity) {   // (whole or not at all; later batches are tried again)
            d->emit_skipped[e]++;
            continue;
        }
        if (timed && !fired) {
            Event mark;
            WGS_TRY(mark.create(hipEventDisableSystemFence));
            HIP_TRY(hipEventRecord(mark, d->stream));
            d->timing.emit_marks.push_back(std::move(mark));
        }
        fired = true;
        const uint32_t model = d->dev.pmodel[0] ? (uint32_t)em.model : (uint32_t)d->dev.model;
        hipLaunchKernelGGL(k_emit<D>, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, d->stream, d->dev, pack_args(d), d->dev.n, (uint32_t)total,
                           em, e, (uint32_t)q, model);
        grew_by(d, (uint32_t)total);
        d->emitted[e] += total;
    }
    if (timed && fired) {
        Event mark;
        WGS_TRY(mark.create(hipEventDisableSystemFence));
        HIP_TRY(hipEventRecord(mark, d->stream));
        d->timing.emit_marks.push_back(std::move(mark));
    }
    if (fired) HIP_TRY(hipGetLastError());
    return WGS_OK;
}

}  // namespace

extern "C" {

wgs_status wgs_data_create_reserved(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                                    size_t num_particles, const wgs_collider *colliders, size_t num_colliders, float cell_width,
                                    uint32_t grid_capacity, uint32_t particle_capacity, wgs_data **out) {
    // (check_create_args raises the capacity to num_particles and holds it to the buffer limit; it adds 64 in 32 bits)
    if (particle_capacity > 0xffffff00u) return fail(WGS_ERR_UNSUPPORTED, "more than ~21M particles per wgs_data: shard across GPUs");
    return create_impl({pipeline, params, particles, num_particles, nullptr, colliders, num_colliders, cell_width,
                        grid_capacity, particle_capacity, false, 0, 0, 0}, out);
}

wgs_status wgs_get_particle_capacity(wgs_data *d, uint32_t *out) {
    if (!d || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = d->capacity;
    return WGS_OK;
}

wgs_status wgs_add_particles(wgs_data *d, const wgs_particle *particles, const uint8_t *models, size_t k) {
    if (!d || (k && !particles)) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_add_particles: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    if (k > (size_t)(d->capacity - d->dev.n))
        return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_add_particles: " + std::to_string(d->dev.n) + " + " + std::to_string(k) + " particles, the capacity is " +
                                                  std::to_string(d->capacity) + " (wgs_data_create_reserved)");
    for (size_t i = 0; i < k; i++) {
        if (models && models[i] > WGS_MODEL_FLUID)
            return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_add_particles: models entry " + std::to_string(i) + " is " + std::to_string((int)models[i]) + ", not a WGS_MODEL_* (0, 1, 2)");
        const std::string problem = layout_problem(d, particles[i], models && models[i] == WGS_MODEL_FLUID);
        if (!problem.empty()) return fail(WGS_ERR_UNSUPPORTED, "wgs_add_particles: particle " + std::to_string(i) + ": " + problem);
    }
    if (k == 0) return WGS_OK;
    WGS_TRY(enter(d));
    const bool table = d->dev.pmodel[0] != nullptr;
    Scratch<wgs_particle> records;
    Scratch<uint8_t> labels;
    WGS_TRY(records.alloc(k));
    HIP_TRY(hipMemcpyAsync(records.ptr, particles, sizeof(wgs_particle) * k, hipMemcpyHostToDevice, d->stream));
    if (table && models) {
        WGS_TRY(labels.alloc(k));
        HIP_TRY(hipMemcpyAsync(labels.ptr, models, k, hipMemcpyHostToDevice, d->stream));
    }
    hipLaunchKernelGGL(k_append<D>, dim3((uint32_t)((k + 255u) / 256u)), dim3(256), 0, d->stream, d->dev, pack_args(d), d->dev.n, (uint32_t)k,
                       records.ptr, labels.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d->stream));   // (the scratch copies are released on return)
    grew_by(d, (uint32_t)k);
    return WGS_OK;
}

wgs_status wgs_set_emitters(wgs_data *d, const wgs_emitter *emitters, uint32_t n) {
    if (!d) return fail(WGS_ERR_INVALID_ARGUMENT, "data is NULL");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_emitters: sharded wgs_data (a slab's particle counts live on the device): single-domain data only");
    if (n > WGS_MAX_EMITTERS) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_emitters: at most WGS_MAX_EMITTERS emitters");
    if (n > 0 && !emitters) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_set_emitters: NULL emitters with n > 0");
    for (uint32_t i = 0; i < n; i++) {
        if (const char *problem = emitter_problem(d, emitters[i])) return fail(WGS_ERR_INVALID_ARGUMENT, std::string(problem) + " (emitter " + std::to_string(i) + ")");
        const std::string mismatch = layout_problem(d, emitters[i].proto, emitters[i].model == WGS_MODEL_FLUID);
        if (!mismatch.empty()) return fail(WGS_ERR_UNSUPPORTED, "wgs_set_emitters: proto of emitter " + std::to_string(i) + ": " + mismatch);
    }
    for (uint32_t i = 0; i < WGS_MAX_EMITTERS; i++) {
        d->emitters[i] = i < n ? emitters[i] : wgs_emitter{};
        d->emitted[i] = d->emit_skipped[i] = 0;
    }
    d->emit_n = n;
    d->emit_set = n > 0;
    return WGS_OK;
}

wgs_status wgs_get_emitters(wgs_data *d, wgs_emitter *out, uint32_t *n) {
    if (!d || !out || !n) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_emitters: sharded wgs_data: single-domain data only");
    for (uint32_t i = 0; i < WGS_MAX_EMITTERS; i++) out[i] = d->emitters[i];
    *n = d->emit_n;
    return WGS_OK;
}

wgs_status wgs_get_emitter_counts(wgs_data *d, uint64_t emitted[WGS_MAX_EMITTERS], uint64_t skipped_batches[WGS_MAX_EMITTERS]) {
    if (!d || !emitted || !skipped_batches) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (d->dev.sharded) return fail(WGS_ERR_UNSUPPORTED, "wgs_get_emitter_counts: sharded wgs_data: single-domain data only");
    for (uint32_t i = 0; i < WGS_MAX_EMITTERS; i++) {
        emitted[i] = d->emitted[i];
        skipped_batches[i] = d->emit_skipped[i];
    }
    return WGS_OK;
}

}  // extern "C"
