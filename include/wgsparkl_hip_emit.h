/*
 * wgsparkl_hip_emit.h — the run-time particle extension of the C ABI (included by wgsparkl_hip.h behind the force-field extension;
 * never on its own: it uses wgs_status, wgs_data, wgs_particle and WGS_DIM of that header).
 *
 * Adding particles at run time. NEW: the reference's MpmData holds the particles it was created with (src/pipeline.rs:98-128). Here a
 * wgs_data may RESERVE particle slots at creation and fill them later, by batches the caller hands over (wgs_add_particles) or by
 * emitters the library fires itself every few substeps (wgs_set_emitters). Both write the new particles into the slots behind the
 * residents of the current buffer, raise the particle count — on single-domain data a host value passed with every launch — and
 * make the next substep rebuild the block table (wgs_stats.table_rebuilds counts it), which bins whatever the buffer holds. No sort,
 * P2G, grid or G2P kernel is involved or changed: data that reserves nothing and adds nothing launches exactly what it launched before.
 * The host always knows the particle count; nothing here synchronises inside wgs_step. Removing particles (sinks, outflow) and
 * appending without a rebuild are not part of this extension.
 *
 * Capacity. wgs_data_create_reserved is wgs_data_create with room for max(num_particles, particle_capacity) particles: every
 * per-particle array is sized by it, and the buffer limit of wgs_data_create (about 21 M particles) applies to it. num_particles == 0
 * is allowed: such data uses the general (non-uniform) layouts and carries no plastic state. wgs_get_particle_capacity answers the
 * reservation (data of wgs_data_create: its particle count).
 *
 * wgs_add_particles. Blocking, like wgs_set_plastic_state. The k new particles get the caller's indices num_particles ..
 * num_particles + k - 1, in the order given: every reader that answers "in the caller's order" (positions, particles, models, particle
 * fields, the vertex buffer, diagnostics, wgs_stats.num_particles) includes them from the return of the call on, before any substep.
 * A new particle is stored as wgs_data_create stores it: the same defaults for has_plasticity == 0 / has_phase == 0, the plastic state
 * {1, 1, 0}, its cdf taken as the input's. `models` (k bytes, WGS_MODEL_*) is READ only while a per-particle model table is set
 * (wgs_set_particle_models); NULL then means the data's model. A particle labelled WGS_MODEL_FLUID, or any particle of data under that
 * model, has its def_grad stored as diag(det F, 1[, 1]), exactly as creation followed by the selector does.
 *
 * Emitters. An emitter is an axis-aligned lattice box of prod(count) particles, emitted again every `period` substeps; up to
 * WGS_MAX_EMITTERS per wgs_data. `proto` is the particle: everything but its position is copied, dynamics.velocity is the emission
 * velocity; `model` is read as the `models` byte of wgs_add_particles.
 *
 *   Schedule. In front of the substep whose wgs_stats.substeps_done value is s, emitter e emits batch number
 *     q = (s - start_substep) / period     if  s >= start_substep,  (s - start_substep) % period == 0  and  (q < batches or batches == 0).
 *   Emitters fire in array order. Integer arithmetic on the host inside wgs_step, timestamped steps included. A batch that would not
 *   fit WHOLE into the remaining capacity is skipped and counted (skipped_batches); nothing else happens — no error bit, the run goes
 *   on —, and later batches are tried again.
 *
 *   Positions. Point i = (i_0, ..) of a batch, point_index = i_0 + count[0] * (i_1 + count[1] * i_2) (x fastest), sits at
 *     x_k = fl(fl(lo_k + fl(fl((float)i_k + 0.5f) * spacing)) + fl(fl(jitter * spacing) * u_k))
 *   every fl() a rounding of its own (no contraction), with
 *     u_k  = (float)(hash >> 8) * 2^-24 - 0.5f          in [-0.5, 0.5)
 *     hash = wgs_lowbias32(seed ^ wgs_lowbias32(q * 0x9E3779B9u + e) ^ wgs_lowbias32(point_index * WGS_DIM + k))
 *   e the emitter's index in the array, q the batch number; uint32 arithmetic modulo 2^32. wgs_lowbias32 is written out below.
 *
 *   The particles of a batch get the indices num_particles .. in point_index order. A substep in which some emitter fired rebuilds the
 *   block table like wgs_add_particles; the time of the emitting launch is reported under WGS_PASS_GRID_SORT. wgs_set_emitters replaces
 *   the whole set and zeroes the counters of wgs_get_emitter_counts: emitted[e] = PARTICLES emitter e has emitted, skipped_batches[e] =
 *   batches it skipped for lack of room. n == 0 removes every emitter. The emitters are host state of the handle (no device memory, not
 *   part of a checkpoint).
 *
 * Errors (refusals change nothing). WGS_ERR_INVALID_ARGUMENT: NULL data, out or particles (with k > 0) / emitters (with n > 0);
 * num_particles + k, or one batch of an emitter, beyond the capacity; a model byte > 2; period == 0; a count of 0; jitter outside
 * [0, 0.5] or not finite; spacing not finite; n > WGS_MAX_EMITTERS. WGS_ERR_UNSUPPORTED: sharded data (wgs_data_create_sharded: a slab's
 * particle counts live on the device); a particle or proto the data's layout cannot hold, with a message that names the mismatch — a
 * plastic or phase-carrying particle (one for which wgs_data_create would have switched the plastic step on) on data whose step carries
 * no plastic state, a WGS_MODEL_FLUID label on data that carries it, a particle whose (mass, init_volume, lambda, mu) differ bitwise
 * from the uniform-material constants the data was created under, or whose plasticity parameters differ bitwise from its uniform ones.
 */
#ifndef WGSPARKL_HIP_EMIT_H
#define WGSPARKL_HIP_EMIT_H

#if defined(__HIP__) || defined(__CUDACC__)
#define WGSPARKL_EMIT_FN static inline __host__ __device__
#else
#define WGSPARKL_EMIT_FN static inline
#endif
/* The integer mixer of the jitter (the "lowbias32" constants): the one definition host, device and bindings restate. */
WGSPARKL_EMIT_FN uint32_t wgs_lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352dU;
    x ^= x >> 15;
    x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}
#undef WGSPARKL_EMIT_FN

#define WGS_MAX_EMITTERS 8
typedef struct {   /* 240 bytes in 3D, 176 in 2D */
    wgs_particle proto;
    uint8_t model;
    float lo[WGS_DIM];
    uint32_t count[WGS_DIM];
    float spacing;
    float jitter;
    uint32_t seed;
    uint32_t start_substep, period, batches;
} wgs_emitter;

wgs_status wgs_data_create_reserved(wgs_pipeline *pipeline, const wgs_sim_params *params, const wgs_particle *particles,
                                    size_t num_particles, const wgs_collider *colliders, size_t num_colliders, float cell_width,
                                    uint32_t grid_capacity, uint32_t particle_capacity, wgs_data **out);
wgs_status wgs_get_particle_capacity(wgs_data *data, uint32_t *out);
wgs_status wgs_add_particles(wgs_data *data, const wgs_particle *particles, const uint8_t *models /* k bytes or NULL */, size_t k);
wgs_status wgs_set_emitters(wgs_data *data, const wgs_emitter *emitters /* n, or NULL with n == 0 */, uint32_t n);
wgs_status wgs_get_emitters(wgs_data *data, wgs_emitter *out /* WGS_MAX_EMITTERS */, uint32_t *n);
wgs_status wgs_get_emitter_counts(wgs_data *data, uint64_t emitted[WGS_MAX_EMITTERS], uint64_t skipped_batches[WGS_MAX_EMITTERS]);

#endif
