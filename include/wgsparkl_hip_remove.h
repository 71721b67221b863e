/*
 * wgsparkl_hip_remove.h — the particle-removal extension of the C ABI (included by wgsparkl_hip.h behind the run-time particle
 * extension; never on its own: it uses wgs_status, wgs_data, wgs_pipeline and WGS_DIM of that header and WGS_REGION_BOX / WGS_REGION_BALL
 * of wgsparkl_hip_forces.h).
 *
 * Removing particles at run time: the other half of wgsparkl_hip_emit.h. NEW: the reference's MpmData holds the particles it was created
 * with (src/pipeline.rs:98-128). Here particles leave a wgs_data by a mask the caller hands over (wgs_remove_particles, or
 * wgs_remove_particles_device with the mask in device memory), by regions evaluated on the device now (wgs_remove_particles_in), or by
 * up to WGS_MAX_SINKS sinks the library evaluates itself every few substeps (wgs_set_sinks). All of them do the same thing: the
 * survivors are gathered into the front slots of the particle buffer, their ids are renumbered densely, the particle count shrinks and
 * the next substep rebuilds the block table (wgs_stats.table_rebuilds counts it), as after wgs_add_particles. No sort, P2G, grid or G2P
 * kernel is involved or changed: data that removes nothing and has no sinks launches exactly what it launched before.
 *
 * A removal is decided on the device, so the host has to ASK for the new particle count: the mask forms read four bytes back (the
 * total of the keep-scan), the region forms and the sinks the WGS_MAX_SINKS per-sink counts, 32 bytes, whose sum is the number
 * removed. The explicit calls are Blocking, like wgs_add_particles. A scheduled sink synchronises the data's stream inside wgs_step, but only in
 * front of the substeps in which some sink is due: `period` is the lever.
 *
 * Renumbering. Survivors keep their relative caller order: the new index of a survivor is its old index minus the number of removed
 * particles in front of it. Every reader that answers "in the caller's order" (positions, particles and plastic state, models, particle
 * fields, the vertex buffer, diagnostics, wgs_stats.num_particles) answers the survivors under the new indices from the return of the
 * call on, before any substep. `kept_from` (may be NULL; otherwise room for the OLD num_particles entries) receives, for every new
 * index i < new num_particles, the old index of that particle: kept_from is increasing, and a caller compacts per-particle arrays of
 * their own by old[kept_from]. `num_removed` receives the number of particles removed. The vacated slots hold what a reserved, never
 * filled slot holds after wgs_data_create_reserved: removing and then adding is adding to data created from the survivors.
 *
 * wgs_remove_particles. `remove`: num_particles bytes in the caller's order, nonzero = remove. Removing every particle is allowed.
 * wgs_remove_particles_device is the same with `remove` AND `kept_from` (or NULL) in device memory, read and written on the data's
 * stream — a mask computed from wgs_read_particle_fields_device, say; it returns the count, so it blocks too.
 *
 * Regions. A wgs_sink is a region and a side; the schedule fields are read by wgs_set_sinks only (wgs_remove_particles_in ignores
 * them). The struct is the same in both dimensions: the third components are ignored in 2D.
 *   Membership is evaluated in fp32 from the position the current buffer stores — the value wgs_read_positions answers —, with
 *   d_k = fl(x_k - center_k), k < WGS_DIM, every fl() a rounding of its own (no contraction):
 *     WGS_REGION_BOX   inside  <=>  fabsf(d_k) <= half_k on every axis k < WGS_DIM;
 *     WGS_REGION_BALL  inside  <=>  s <= fl(half_0 * half_0), s = fl(d_0 * d_0); s = fl(s + fl(d_1 * d_1)); [3D: s = fl(s + fl(d_2 * d_2));]
 *   (a disc in 2D). On a face (==) counts as inside. A comparison with a NaN is false: a particle with a non-finite position is inside
 *   nothing. WGS_REGION_ALL is refused.
 *   WGS_SINK_INSIDE removes the particles inside the region, WGS_SINK_OUTSIDE the particles that are NOT inside it — an outflow
 *   boundary, "everything that leaves this box"; it takes a particle with a NaN position.
 *   A particle that several sinks of one call or pass would remove counts for the first of them in array order.
 *
 * Sinks. wgs_set_sinks replaces the whole set and zeroes the counters of wgs_get_sink_counts: removed[e] = particles sink e has
 * removed. n == 0 removes every sink. The sinks are host state of the handle (no device memory: wgs_stats.device_bytes does not
 * change; not part of a checkpoint).
 *   Schedule. In front of the substep whose wgs_stats.substeps_done value is s, sink e is due if
 *     s >= start_substep  and  (s - start_substep) % period == 0.
 *   All due sinks are evaluated in ONE pass, in front of the emitters of that substep (wgsparkl_hip_emit.h): the room they free is
 *   available to those emitters. A pass costs one stream synchronisation and a read of the counters, and — the sinks owning no device
 *   memory — one allocation of num_particles bytes and its release, which waits for the device: a few tens of microseconds per pass at 1 M and
 *   at 2 M particles on an MI355X (notes/round_35.md has the figures). A pass that removes nothing does
 *   nothing else — no rebuild, no write: the run stays bit-identical to one without sinks, wgs_stats.table_rebuilds included. A pass that
 *   removes something makes that substep rebuild the block table like wgs_add_particles; with timestamps its time is reported under
 *   WGS_PASS_GRID_SORT.
 *
 * Errors (refusals change nothing). WGS_ERR_INVALID_ARGUMENT: a NULL data, remove, regions (with n > 0), num_removed, out or counter
 * array; n > WGS_MAX_SINKS; a region that is not WGS_REGION_BOX or WGS_REGION_BALL; side > 1; period == 0 in wgs_set_sinks; a
 * non-finite center component, or a negative or non-finite half component, that the region reads (BOX: the first WGS_DIM of each,
 * BALL: the first WGS_DIM of center and half[0]). WGS_ERR_UNSUPPORTED: sharded data (wgs_data_create_sharded: a slab's particle counts
 * live on the device).
 *
 * Not part of this extension: removal on sharded data; removal without a table rebuild; sinks that need no synchronisation; sinks
 * that depend on the velocity or on a field — the mask forms cover those from the caller's side.
 */
#ifndef WGSPARKL_HIP_REMOVE_H
#define WGSPARKL_HIP_REMOVE_H

#define WGS_MAX_SINKS 8
enum { WGS_SINK_INSIDE = 0, WGS_SINK_OUTSIDE = 1 };
typedef struct {   /* 40 bytes */
    uint32_t region;   /* WGS_REGION_BOX or WGS_REGION_BALL */
    uint32_t side;     /* WGS_SINK_INSIDE or WGS_SINK_OUTSIDE */
    float center[3];
    float half[3];     /* BOX: half extents; BALL: half[0] is the radius */
    uint32_t start_substep, period;
} wgs_sink;

wgs_status wgs_remove_particles(wgs_data *data, const uint8_t *remove, uint32_t *kept_from /* or NULL */, uint32_t *num_removed);
wgs_status wgs_remove_particles_device(wgs_data *data, const uint8_t *remove_device, uint32_t *kept_from_device /* or NULL */, uint32_t *num_removed);
wgs_status wgs_remove_particles_in(wgs_data *data, const wgs_sink *regions, uint32_t n, uint32_t *kept_from /* or NULL */, uint32_t *num_removed);
wgs_status wgs_set_sinks(wgs_data *data, const wgs_sink *sinks /* n, or NULL with n == 0 */, uint32_t n);
wgs_status wgs_get_sinks(wgs_data *data, wgs_sink *out /* WGS_MAX_SINKS */, uint32_t *n);
wgs_status wgs_get_sink_counts(wgs_data *data, uint64_t removed[WGS_MAX_SINKS]);
/* TEST HOOK (not part of the drop-in surface), like wgs_debug_scan: the keep-scan of a removal alone, on caller arrays.
 * new_index[i] = number of i' < i with remove[i'] == 0 (n entries), *kept (may be NULL) = number of zeros in all. Blocking. */
wgs_status wgs_debug_compact_map(wgs_pipeline *pipeline, const uint8_t *remove, uint32_t n, uint32_t *new_index, uint32_t *kept);

#endif
