/*
 * wgsparkl_hip_forces.h — the force-field extension of the C ABI (included by wgsparkl_hip.h behind its plasticity section; never
 * on its own: it uses wgs_status, wgs_data and WGS_DIM of that header).
 *
 * Force fields. NEW: the reference's only body force is SimulationParams::gravity, one vector for the whole domain
 * (src/solver/params.rs:6-16). A force field is a rule on the grid NODES' velocities, applied once per substep in a short launch of its
 * own behind the grid update (either form of it) and IN FRONT OF the domain walls and the fused G2P: a wall's postconditions keep
 * holding whatever the fields do. Up to WGS_MAX_FORCE_FIELDS per wgs_data; they apply in array order, each on the running value.
 * Only nodes of active blocks with mass > 0 are touched; a node's mass is never touched; a node whose velocity bits do not change is
 * not written. Data without fields launches exactly what it launched before.
 *
 * The rule.
 *   x  = node position in world units. x_k = (float)cell_k * h, with cell_k = block_k * BW + local_k — the integers wgs_read_grid
 *        reports in wgs_node_record.cell, h the cell width of wgs_data_create.
 *   dt = the device's SimParamsDev::dt, as the grid update reads it. wgs_set_sim_params carries over.
 *
 *   w_p(q), p = falloff in {0,1,2,3}:   1,  1/sqrt(q),  1/q,  1/(q sqrt(q))
 *
 *   UNIFORM  v += dt * vec
 *   RADIAL   r = center - x;  q = |r|^2 + softening^2;   v += dt * strength * w_p(q) * r      (strength > 0 attracts)
 *   VORTEX   r = x - center;  rp = r - (r.n) n;  q = |rp|^2 + softening^2;
 *            v += dt * strength * w_p(q) * (n x rp)
 *            3D: n = vec normalised once on the host in double
 *            2D: n = +z, i.e. (-r_y, r_x)
 *   DRAG     kdt = min(strength * dt, 1e30);  s = kdt / (1 + kdt);  v += s * (vec - v)
 *            backward Euler relaxation toward the velocity `vec`:
 *            stable for any rate; a large rate prescribes the velocity
 *
 * All in fp32 on the device. The normalised n of a 3D VORTEX is rounded to fp32 once, component by component, and is what
 * wgs_get_force_fields does NOT report: the getter answers the caller's own `vec`. DRAG is evaluated as v = (1 - s) v + s vec, the same
 * number: s == 1 (strength * dt >= 2^25) then leaves `vec` bit for bit. 1/sqrt(q) is a correctly rounded root and a correctly rounded
 * quotient, never a hardware approximation.
 *
 * Regions. Every field acts only on the nodes inside its region:
 *   WGS_REGION_ALL   every node;
 *   WGS_REGION_BOX   |x_k - region_center_k| <= region_half_k on every axis;
 *   WGS_REGION_BALL  |x - region_center|^2 <= region_half[0]^2. This is a disc in 2D. (The device also asks |x_k - region_center_k| <=
 *                    region_half[0] on every axis — implied in exact arithmetic — so that the ball lies inside its bounding box in
 *                    fp32 too: a block is skipped on its key alone when its node box misses the bounding box of every region.)
 * Membership is decided in fp32 from x as above; a caller who needs it exact puts region faces half-way between nodes, at (k + 1/2) h.
 *
 * The same 68-byte struct in both dimensions; the third components are ignored by the 2D library. `kind == WGS_FORCE_NONE` entries
 * are kept and skipped. `n == 0` removes every field. Stream-ordered like the other setters: the substeps enqueued after the call use
 * it. Like the walls, the fields are host state of the handle and travel as a kernel argument: they take no device memory
 * (wgs_stats.device_bytes does not change), nothing in the device's argument block, no upload, and they are NOT part of a checkpoint
 * (wgs_read_particles -> wgs_data_create restarts without them: set them again). Time-dependent or moving fields: set them again
 * between wgs_step calls. wgs_read_grid, wgs_sample_grid, wgs_read_grid_window and the WGS_DIAG_GRID sums see the velocities AFTER the
 * fields (and after the walls); the time of the launch is reported under WGS_PASS_GRID_UPDATE. WGS_SUM_GRAVITY_POTENTIAL stays
 * gravity's: the fields have no energy sum. Colliders, walls, per-particle models and either plasticity rule may be used together with
 * fields: the fields act on the node values all of them read.
 *
 * Errors (refusals change nothing: wgs_get_force_fields then answers what it answered before). WGS_ERR_INVALID_ARGUMENT: n >
 * WGS_MAX_FORCE_FIELDS; NULL fields with n > 0; NULL data, out or n; kind > 4, falloff > 3 or region > 2; any non-finite float in a
 * field whose kind is not WGS_FORCE_NONE; softening < 0; softening == 0 with falloff > 0 on RADIAL or VORTEX (the centre would be a
 * pole); strength < 0 on DRAG; a negative region_half component that the region reads (BOX: the first WGS_DIM, BALL: the first);
 * a VORTEX with |vec| == 0 in 3D. WGS_ERR_UNSUPPORTED: sharded data (wgs_data_create_sharded), like wgs_set_domain_walls.
 */
#ifndef WGSPARKL_HIP_FORCES_H
#define WGSPARKL_HIP_FORCES_H

enum { WGS_FORCE_NONE = 0, WGS_FORCE_UNIFORM = 1, WGS_FORCE_RADIAL = 2, WGS_FORCE_VORTEX = 3, WGS_FORCE_DRAG = 4 };
enum { WGS_REGION_ALL = 0, WGS_REGION_BOX = 1, WGS_REGION_BALL = 2 };
#define WGS_MAX_FORCE_FIELDS 8
typedef struct {   /* the same 68 bytes in both dimensions; the third components are ignored by the 2D library */
    uint32_t kind, falloff, region;
    float strength, softening;
    float center[3], vec[3], region_center[3], region_half[3];
} wgs_force_field;
wgs_status wgs_set_force_fields(wgs_data *data, const wgs_force_field *fields /* n, or NULL with n == 0 */, uint32_t n);
wgs_status wgs_get_force_fields(wgs_data *data, wgs_force_field *out /* WGS_MAX_FORCE_FIELDS */, uint32_t *n);

#endif
