/*
 * wgsparkl_hip.h — C ABI of the MI355X-native MLS-MPM step (drop-in for the
 * one hot path of dimforge/wgsparkl: `MpmPipeline::queue_step`).
 *
 * Build twice, like the reference builds its two crates from one source tree
 * (Cargo.toml:1-8): -DWGS_DIM=3 -> libwgsparkl3d_hip.so, -DWGS_DIM=2 ->
 * libwgsparkl2d_hip.so. Both export the same symbol names.
 *
 * Every entry point cites the reference interface it replaces (paths relative
 * to /root/reference). Plain pointers and sizes only; no exceptions cross the
 * boundary; every call returns a wgs_status (0 = ok) and leaves a message for
 * wgs_last_error(). Handles are not internally synchronised: one host thread
 * per wgs_data at a time (the reference calls from one Bevy system,
 * src_testbed/lib.rs:60-69).
 */
#ifndef WGSPARKL_HIP_H
#define WGSPARKL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifndef WGS_DIM
#define WGS_DIM 3
#endif

#if WGS_DIM == 2
#define WGS_ANG_DIM 1
#else
#define WGS_ANG_DIM 3
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t wgs_status;
enum {
    WGS_OK = 0,
    WGS_ERR_INVALID_ARGUMENT = 1,
    WGS_ERR_NO_DEVICE = 2,       /* no HIP device / HIP runtime failure at creation */
    WGS_ERR_HIP = 3,             /* a HIP call failed; see wgs_last_error() */
    WGS_ERR_GRID_OVERFLOW = 4,   /* more active blocks than grid_capacity (the reference drops them silently, src/grid/grid.wgsl:126-128,163) */
    WGS_ERR_KEY_RANGE = 5,       /* a block left the packed-key range (src/grid/grid.wgsl:88-95; quirk B5) */
    WGS_ERR_UNSUPPORTED = 6
};

/* src/solver/params.rs:6-16 SimulationParams (2D: gravity[2]; the f32 padding is not exposed). */
typedef struct {
    float gravity[WGS_DIM];
    float dt;
} wgs_sim_params;

/* src/models/mod.rs:65-70 ElasticCoefficients */
typedef struct { float lambda, mu; } wgs_elastic_coefficients;
/* src/models/drucker_prager.rs:6-15 DruckerPrager */
typedef struct { float h0, h1, h2, h3, lambda, mu; } wgs_drucker_prager;
/* src/models/drucker_prager.rs:36-42 DruckerPragerPlasticState */
typedef struct { float plastic_deformation_gradient_det, plastic_hardening, log_vol_gain; } wgs_plastic_state;
/* src/solver/particle_update.rs:35-40 ParticlePhase */
typedef struct { float phase, max_stretch; } wgs_particle_phase;

/* src/solver/particle3d.rs:44-51 / particle2d.rs:42-49 Cdf */
typedef struct {
    float normal[WGS_DIM];
    float rigid_vel[WGS_DIM];
    float signed_distance;
    uint32_t affinity;
} wgs_cdf;

/* src/solver/particle3d.rs:16-26 ParticleDynamics, Rust field order; matrices column-major (nalgebra). */
typedef struct {
    float velocity[WGS_DIM];
    float def_grad[WGS_DIM * WGS_DIM];
    float affine[WGS_DIM * WGS_DIM];
    wgs_cdf cdf;
    float init_volume;
    float init_radius;
    float mass;
} wgs_particle_dynamics;

/* src/solver/particle3d.rs:53-60 Particle. Option<T> is flattened to has_* + value;
 * has_* == 0 applies the reference defaults of src/models/mod.rs:24,33-36. */
typedef struct {
    float position[WGS_DIM];
    wgs_particle_dynamics dynamics;
    wgs_elastic_coefficients model;
    uint32_t has_plasticity;
    wgs_drucker_prager plasticity;
    uint32_t has_phase;
    wgs_particle_phase phase;
} wgs_particle;

/* One coupled collider: what MpmData::new keeps of rapier's (RigidBody, Collider)
 * pair (src/pipeline.rs:107-117 -> wgrapier GpuBodySet: shape, pose, velocity,
 * world mass properties). Only analytic shapes are handled, like collide()
 * (src/collision/collide.wgsl:36-38 skips polylines and trimeshes). */
enum { WGS_SHAPE_BALL = 0, WGS_SHAPE_CUBOID = 1, WGS_SHAPE_CAPSULE = 2,
       WGS_SHAPE_MESH = 3 /* trimesh / heightfield / polyline: no analytic projection, coupled through the rigid
                             particles of wgs_set_rigid_particles */ };
typedef struct {
    float rotation[4];     /* 3D: unit quaternion (i, j, k, w); 2D: (cos, sin, 0, 0) */
    float translation[3];
    float scale;
} wgs_pose;                /* wgebra Sim3 / Sim2 */
typedef struct {
    float linear[3];
    float angular[3];      /* 2D: angular[0] */
} wgs_velocity;            /* wgrapier Body::Velocity */
typedef struct {
    uint32_t shape_type;   /* WGS_SHAPE_* */
    float shape[4];        /* ball: r | cuboid: half extents | capsule: half height (local y), r */
    wgs_pose pose;
    wgs_velocity velocity;
    float com[3];          /* world-space centre of mass (wgrapier MassProperties.com) */
} wgs_collider;
#define WGS_MAX_COLLIDERS 16 /* src/grid/grid.wgsl:230-240: 16 affinity + 16 sign bits */
/* Mass properties of the rigid body behind a collider (wgrapier GpuBodySet local_mprops, bound at
 * src/solver/rigid_impulses.wgsl:81-84). All zero (the default) = kinematic or fixed body: it follows its
 * velocity. Non-zero = dynamic: the particles push it back (two-way coupling, src/solver/p2g.wgsl:200-228,
 * src/solver/rigid_impulses.wgsl:95-136). The centre of mass is wgs_collider.com. */
typedef struct {
    float inv_mass[3];           /* per-axis inverse mass */
    float inv_inertia_local[9];  /* 3D: column-major inverse inertia tensor in the body frame; 2D: [0] = 1/I */
} wgs_mass_properties;

/* Constitutive model (the reference picks at shader-compile time,
 * src/solver/particle_update.wgsl:7-8; default = corotated like the reference). */
enum { WGS_MODEL_COROTATED = 0, WGS_MODEL_NEO_HOOKEAN = 1, WGS_MODEL_FLUID = 2 };
/* WGS_MODEL_FLUID — weakly-compressible fluid: Tait pressure + Newtonian viscosity. NEW: the reference ships no fluid / equation of
 * state. The only deformation state of a particle is its volume ratio J. Per particle and substep, with G = the velocity gradient
 * G2P leaves in `affine` (src/solver/particle_update.wgsl:89-91), lambda, mu = the particle's wgs_elastic_coefficients REINTERPRETED
 * (lambda = bulk modulus at rest, mu = dynamic viscosity), gamma = the Tait exponent of wgs_set_fluid_eos:
 *     J'      = J * det(I + dt * G)                  the determinant of what F <- F + (G dt) F does to an isotropic F
 *     Jc      = max(J', 1e-10)                       the clamp of src/models/neo_hookean_elasticity.wgsl:14-25
 *     p       = (lambda / gamma) * (Jc^(-gamma) - 1) Tait; dp/dJ = -lambda at J = 1
 *     tau     = -Jc * p * I + Jc * mu * (G + G^T)    Kirchhoff stress = J * Cauchy stress
 *     affine' = G * m - tau * (V0 * inv_d * dt)      src/solver/particle_update.wgsl:129-132, unchanged
 * Advection, the velocity clamp, the CPIC projection and the penalty impulse are those of the other models. To first order in J - 1
 * the pressure term is the lambda ln J of the neo-Hookean model with mu = 0.
 * def_grad of a fluid particle is NOT a deformation gradient: it is diag(J, 1[, 1]) — entry [0] holds J, the rest is the identity —,
 * whose determinant is J exactly, so wgs_read_particles -> wgs_data_create -> wgs_set_constitutive_model(FLUID) restarts a run bit for
 * bit and every diagnostic that takes det F works as it is. wgs_prep_vertex_buffer* draws a fluid particle with cbrt(J) I (2D: sqrt(J) I).
 * Selecting the model is stream-ordered: it enqueues one small kernel that collapses the def_grad of every particle to
 * diag(det F, 1[, 1]) (nothing changes where it has that form already); selecting another model afterwards needs nothing. On data
 * whose step carries plastic state (Drucker-Prager particles, breakable phases, force_plastic) the call returns WGS_ERR_UNSUPPORTED
 * and changes nothing. */
/* Per-particle models (wgs_set_particle_models below): what wgs_diagnostics.model reports while a table is set. Never a model of its
 * own: wgs_set_constitutive_model refuses it like any other unknown value. */
#define WGS_MODEL_PER_PARTICLE 3

/* The reference's 10 timestamped passes (src/pipeline.rs:201-271). The fused
 * G2P + particle update reports its time under WGS_PASS_G2P; in collider simulations
 * the same kernel's second launch, over the blocks near a collider, is reported under
 * WGS_PASS_PARTICLES_UPDATE (0 without colliders). */
enum {
    WGS_PASS_UPDATE_RIGID_PARTICLES = 0, WGS_PASS_GRID_SORT = 1, WGS_PASS_GRID_UPDATE_CDF = 2,
    WGS_PASS_P2G_CDF = 3, WGS_PASS_G2P_CDF = 4, WGS_PASS_P2G = 5, WGS_PASS_GRID_UPDATE = 6,
    WGS_PASS_G2P = 7, WGS_PASS_PARTICLES_UPDATE = 8, WGS_PASS_INTEGRATE_BODIES = 9,
    WGS_NUM_PASSES = 10
};

/* Grid node keyed by world cell coordinate (active blocks are numbered by an
 * atomic counter in the reference, src/grid/grid.wgsl:327, so physical ids are
 * not comparable between runs; virtual ids are). */
typedef struct {
    int32_t cell[WGS_DIM];
    float velocity[WGS_DIM];   /* momentum_velocity_mass.xyz after the grid update */
    float mass;
    float cdf_distance;
    uint32_t cdf_affinities;
    uint32_t cdf_closest_id;
} wgs_node_record;

/* src/grid/grid.rs:250-256 GpuActiveBlockHeader */
typedef struct {
    int32_t virtual_id[WGS_DIM];
    uint32_t first_particle;
    uint32_t num_particles;
} wgs_block_record;

typedef struct {
    uint32_t num_particles;
    uint32_t num_active_blocks;   /* of the last executed substep */
    uint32_t grid_capacity;       /* rounded up to a power of two like src/grid/grid.rs:283; grows, see wgs_set_grid_growth */
    uint32_t overflow;            /* sticky: WGS_ERR_GRID_OVERFLOW / WGS_ERR_KEY_RANGE seen on device */
    uint64_t substeps_done;
    uint64_t device_bytes;        /* HBM held by this wgs_data */
    uint32_t num_near_collider_blocks; /* particle-bearing blocks whose tile sees a collider (the CPIC passes' list), last substep */
    uint32_t grid_growths;        /* times the block capacity was doubled (wgs_set_grid_growth) */
    uint64_t cell_changers;       /* particles that changed their associated cell since creation (they are what the sort has to move:
                                     the difference of two reads / (particles x substeps) is the mover fraction per substep) */
    uint64_t table_rebuilds;      /* substeps that rebuilt the table of block ids (a full binning pass in front of the sort: the first substep,
                                     every 1024th, after a growth of the grid, when the ids ran out) — with grid_growths, the fixed-cost events
                                     inside a timed region */
    uint32_t block_ids;           /* physical block ids handed out since the last table rebuild (high-water mark; the capacity bounds it) */
    uint32_t block_ids_free;      /* ... of them on the free list: blocks evicted from the table after 8 substeps without activity, their ids reused */
    uint32_t table_marks;         /* table slots marked "evicted" and not yet reused by an insertion */
    uint32_t table_refreshes;     /* times the table was cleared of those marks: the live blocks re-inserted under their own ids, no particle touched */
} wgs_stats;

typedef struct wgs_pipeline wgs_pipeline;
typedef struct wgs_data wgs_data;

/* Thread-local message of the last failing call on this thread. */
const char *wgs_last_error(void);
/* 2 or 3: the dimension this library was built for (cargo features dim2/dim3, src/lib.rs:4-15). */
int32_t wgs_dim(void);
/* Build identification: dimension, target arch and — never in a shipped library — "WGS_ABLATE" when the kernels were
 * compiled with their ablation switches (bench.py refuses such a build). */
const char *wgs_build_info(void);
/* Version of this header's structs and entry points as the LIBRARY was built (WGS_ABI_VERSION as the caller was): the structs carry no
 * size field — wgs_get_stats writes sizeof(wgs_stats) of ITS header —, so a binding checks wgs_abi_version() == WGS_ABI_VERSION once,
 * after loading the library, and refuses to go on otherwise (include/wgsparkl_hip.hpp and wgsparkl_amd/_ffi.py do). History: 5 =
 * wgs_stats grew by block_ids .. table_refreshes (24 bytes); 6 = this function. New counters will come behind a call of their own.
 * 7 = wgs_read_diagnostics / wgs_enqueue_diagnostics and their structs (nothing that existed changed). Still 7: WGS_MODEL_FLUID and
 * wgs_set_fluid_eos were added without touching a struct, an enum value or a signature — a binding that must run against older
 * libraries of version 7 detects wgs_set_fluid_eos by symbol lookup. Still 7: WGS_MODEL_PER_PARTICLE, wgs_set_particle_models and
 * wgs_read_particle_models were added the same way (new symbols and a macro only; wgs_diagnostics.model may now read 3) — detect
 * wgs_set_particle_models by symbol lookup. Still 7: wgs_grid_sample, wgs_sample_grid[_device] and wgs_read_grid_window[_device] were
 * added the same way (one new struct and four new symbols) — detect wgs_sample_grid by symbol lookup. Still 7: wgs_particle_field and
 * wgs_read_particle_fields[_device] were added the same way (one new struct and two new symbols) —
 * detect wgs_read_particle_fields by symbol lookup. Still 7: wgs_wall and wgs_set_domain_walls / wgs_get_domain_walls were added the
 * same way (one new struct, one enum and two new symbols) — detect wgs_set_domain_walls by symbol lookup. Still 7: WGS_PLASTICITY_*
 * and wgs_set_plasticity_model / wgs_get_plasticity_model were added the same way (one enum and two new symbols) — detect
 * wgs_set_plasticity_model by symbol lookup and, still 7, the force-field extension of wgsparkl_hip_forces.h — detect
 * wgs_set_force_fields by symbol lookup and, still 7, the run-time particle extension of wgsparkl_hip_emit.h (reserved capacity,
 * appended batches, emitters) — detect wgs_add_particles by symbol lookup and, still 7, the particle-removal extension of
 * wgsparkl_hip_remove.h (masks, regions, scheduled sinks) — detect wgs_remove_particles by symbol lookup. */
#define WGS_ABI_VERSION 7
uint32_t wgs_abi_version(void);

/* MpmPipeline::new(&Device) -> Result<Self, ComposerError>  (src/pipeline.rs:176-193).
 * Binds to HIP device `hip_device`; fails with WGS_ERR_NO_DEVICE when there is none
 * (there is no CPU fallback). */
wgs_status wgs_pipeline_create(int32_t hip_device, wgs_pipeline **out);
void wgs_pipeline_destroy(wgs_pipeline *pipeline);

/* MpmData::new(device, params, &[Particle], &RigidBodySet, &ColliderSet, cell_width, grid_capacity)
 * (src/pipeline.rs:98-128). `particles`/`colliders` are borrowed for the call only. */
wgs_status wgs_data_create(wgs_pipeline *pipeline, const wgs_sim_params *params,
                           const wgs_particle *particles, size_t num_particles,
                           const wgs_collider *colliders, size_t num_colliders,
                           float cell_width, uint32_t grid_capacity, wgs_data **out);
void wgs_data_destroy(wgs_data *data);

/* Runtime replacement for the compile-time import at src/solver/particle_update.wgsl:7-8. */
wgs_status wgs_set_constitutive_model(wgs_data *data, int32_t model);
/* The Tait exponent of WGS_MODEL_FLUID (default 7), one value per wgs_data. Stream-ordered like the other setters: the substeps
 * enqueued after the call use it. gamma must be finite and > 1, else WGS_ERR_INVALID_ARGUMENT; allowed under any model, read only
 * by the fluid. */
wgs_status wgs_set_fluid_eos(wgs_data *data, float gamma);
/* Per-particle constitutive model. NEW: the reference compiles ONE model into its shader (src/solver/particle_update.wgsl:7-8); here a
 * simulation may mix them, so that an elastic body can be put into the Tait fluid and the two interact through the shared grid.
 * `models`: num_particles bytes in the caller's order, each WGS_MODEL_COROTATED, WGS_MODEL_NEO_HOOKEAN or WGS_MODEL_FLUID. Blocking, like
 * wgs_set_plastic_state. From the next substep on every particle is advanced under its own model (the transfers do not know the
 * model: the stress enters through `affine` alone); the fluid particles share the data's one wgs_set_fluid_eos gamma, and lambda, mu
 * of a particle mean what its OWN model takes them for. The label travels with the particle: wgs_read_particle_models returns it in
 * the caller's order at any time, and wgs_read_particles + wgs_read_particle_models -> wgs_data_create + wgs_set_particle_models
 * restarts a run bit for bit (the state digest does not hash the model).
 * def_grad of the particles labelled WGS_MODEL_FLUID is collapsed to diag(det F, 1[, 1]) by the call, exactly as
 * wgs_set_constitutive_model(WGS_MODEL_FLUID) does for all particles (nothing changes where it has that form already, so setting the
 * same table twice changes no bit); the others are left as they are. A particle RE-LABELLED from the fluid to a solid keeps
 * diag(J, 1[, 1]) as its deformation gradient: a valid F of that volume ratio, but whatever shape the fluid parcel took is forgotten.
 * While a table is set, wgs_diagnostics.model reads WGS_MODEL_PER_PARTICLE, WGS_SUM_ELASTIC takes Psi of each particle's own model, and
 * wgs_prep_vertex_buffer* draws the fluid particles isotropically (cbrt(J) I / sqrt(J) I) and the others with their F.
 * models == NULL drops the table: every particle is advanced under the data's single model again (def_grad is not touched).
 * wgs_set_constitutive_model while a table is set drops the table first, then does what it always does.
 * Errors (nothing is changed): an entry > 2 -> WGS_ERR_INVALID_ARGUMENT; data whose step carries plastic state (the condition under
 * which WGS_MODEL_FLUID is refused) -> WGS_ERR_UNSUPPORTED; sharded data (wgs_data_create_sharded: the migration record carries no
 * model) -> WGS_ERR_UNSUPPORTED. */
wgs_status wgs_set_particle_models(wgs_data *data, const uint8_t *models /* num_particles, or NULL */);
/* The model of every particle in the caller's order (num_particles bytes). Blocking. Without a table every entry is the data's model. */
wgs_status wgs_read_particle_models(wgs_data *data, uint8_t *out);

/* MpmPipeline::queue_step + `for _ in 0..num_substeps { queue.encode(..) }` + submit
 * (src/pipeline.rs:195-281, src_testbed/step.rs:122-128,169): enqueues `num_substeps`
 * substeps on the data's HIP stream and returns without waiting. `timestamps` != 0
 * brackets each pass with HIP events (src/pipeline.rs:201-271 compute_pass(name, add_timestamps)). */
wgs_status wgs_step(wgs_pipeline *pipeline, wgs_data *data, uint32_t num_substeps, int32_t timestamps);
/* device.poll(Maintain::Wait) (src/pipeline.rs:339). Also reports device-side sticky errors. */
wgs_status wgs_sync(wgs_data *data);

/* queue.write_buffer(sim_params) from the UI (src_testbed/ui.rs:91-104) */
wgs_status wgs_set_sim_params(wgs_data *data, const wgs_sim_params *params);
/* queue.write_buffer(bodies.poses()) (src_testbed/step.rs:79-96); com is refreshed by the caller too */
wgs_status wgs_set_collider_poses(wgs_data *data, const wgs_pose *poses, const float *coms /* n*3 or NULL */, size_t n);
/* queue.write_buffer(bodies.vels()) (src_testbed/step.rs:98-119) */
wgs_status wgs_set_body_velocities(wgs_data *data, const wgs_velocity *vels, size_t n);
/* GpuBodySet::from_rapier's local mass properties (src/pipeline.rs:145, wgrapier): which bodies are dynamic.
 * Stream-ordered like the other setters. On sharded data the impulses are reduced over the ranks (wgs_sharded_step). */
wgs_status wgs_set_body_mass_properties(wgs_data *data, const wgs_mass_properties *mprops, size_t n);
/* Rigid particles of the mesh colliders = the buffers GpuRigidParticles::from_rapier builds on the host
 * (src/solver/particle3d.rs:100-150, 2D src/solver/particle2d.rs:75-125; sampling step = cell width,
 * src/pipeline.rs:144) plus the mesh vertex buffers of wgrapier's GpuBodySet: sample points and mesh vertices in
 * the collider's LOCAL frame, per sample the vertex ids of the triangle (2D: segment, vertex[2] unused) it was
 * taken from and its collider. Every substep then runs `update rigid particles`, the rigid-particle block marks
 * and `p2g_cdf` (src/solver/rigid_particle_update.wgsl, src/grid/sort.wgsl:38-86, src/solver/p2g_cdf.wgsl).
 * Copies its inputs; n == 0 removes them. Blocking. On sharded data every rank passes ALL samples (the node cdfs are a
 * function of position and colliders: the two ranks of a face compute the same values for the nodes they share). */
typedef struct { uint32_t vertex[3]; uint32_t collider; } wgs_sample_ids;   /* GpuSampleIds */
wgs_status wgs_set_rigid_particles(wgs_data *data, const float *local_points /* n*DIM */, const wgs_sample_ids *ids, size_t n,
                                   const float *local_vertices /* nv*DIM */, const uint32_t *vertex_collider_ids, size_t nv);
/* poses_staging read-back after the step (src_testbed/step.rs:129-132,175-198): the poses the device
 * integrated (every substep ends with src/solver/rigid_impulses.wgsl:95-136). Blocking. `vels` and `coms`
 * (n*3 floats, world space) may be NULL. */
wgs_status wgs_read_body_poses(wgs_data *data, wgs_pose *poses, wgs_velocity *vels, float *coms, size_t n);

/* positions is the only particle buffer the reference creates COPY_SRC (src/solver/particle3d.rs:197-201).
 * out: num_particles * WGS_DIM floats, in the caller's original particle order. Blocking. */
wgs_status wgs_read_positions(wgs_data *data, float *out);
/* Optional interop view (SURVEY §8b "Ownership": no borrowed device pointers escape except through this call): where the
 * current particle state lives on the device, for a renderer or a coupling code that reads positions without a host round
 * trip (the reference hands its `positions` buffer to the testbed's render pass the same way, src/solver/particle3d.rs:197-201,
 * src_testbed/step.rs:144-163). One float4 per slot — the first WGS_DIM floats are the position — in the SORTED order of the last
 * substep; particle_ids[slot] is the caller's index of the particle in that slot. Read-only; valid until the next call that
 * steps, sets, restores or destroys `data`. Work enqueued on `hip_stream` before this call is what produced the contents:
 * synchronise, or enqueue the reader behind it. Not blocking. Single-domain data. */
typedef struct {
    const float *position_quads;   /* capacity * 4 floats */
    const uint32_t *particle_ids;  /* capacity */
    uint32_t count;                /* slots in use = number of particles */
    uint32_t capacity;
    uint32_t dim;                  /* WGS_DIM of the library */
    uint32_t reserved;
    void *hip_stream;              /* hipStream_t of `data` */
} wgs_device_ptrs;
wgs_status wgs_get_device_ptrs(wgs_data *data, wgs_device_ptrs *out);
/* Full particle state in the caller's original order (tests / checkpoint). Blocking. */
wgs_status wgs_read_particles(wgs_data *data, wgs_particle *out, wgs_plastic_state *plastic_out /* may be NULL */);
/* Render hand-off: src_testbed/prep_vertex_buffer{2,3}d.wgsl `main`, the compute pass the testbed
 * queues after the substeps (src_testbed/step.rs:144-163). One InstanceData per particle in the caller's order
 * (src_testbed/instancing3d.rs:66-74): base_color is an INPUT (set once at startup by the testbed), the rest is
 * written. Modes = RenderMode (src_testbed/prep_vertex_buffer.rs:11-18). */
enum {
    WGS_RENDER_DEFAULT = 0, WGS_RENDER_VOLUME = 1, WGS_RENDER_VELOCITY = 2, WGS_RENDER_CDF_NORMALS = 3,
    WGS_RENDER_CDF_DISTANCES = 4, WGS_RENDER_CDF_SIGNS = 5
};
typedef struct {
    float deformation[3][4]; /* mat3x3 columns, padded to vec4 (2D: F in the xy block, identity elsewhere) */
    float position[4];       /* xyz, 0 (2D: z = 0) */
    float base_color[4];
    float color[4];
} wgs_instance;
/* host buffer of n records: staged to the device, filled, copied back. Blocking. */
wgs_status wgs_prep_vertex_buffer(wgs_data *data, uint32_t mode, wgs_instance *instances);
/* interop form: `device_instances` is a DEVICE pointer to n records that stay resident (the testbed's vertex
 * buffer); stream-ordered, returns immediately. */
wgs_status wgs_prep_vertex_buffer_device(wgs_data *data, uint32_t mode, wgs_instance *device_instances);

/* Checkpoint restore (the reference has no checkpointing, MpmData::new always starts from
 * DruckerPragerPlasticState::default, src/models/drucker_prager.rs:36-53): wgs_read_particles +
 * wgs_read_body_poses -> wgs_data_create (+ wgs_set_body_mass_properties) -> wgs_set_plastic_state continues a
 * run bit-exactly. `states`: one record per particle in the caller's order. Blocking; single-domain data. */
wgs_status wgs_set_plastic_state(wgs_data *data, const wgs_plastic_state *states);
/* Sparse grid of the last substep: nodes of every active block. *count receives the number written. */
wgs_status wgs_read_grid(wgs_data *data, wgs_node_record *out, size_t capacity, size_t *count);
/* Active block headers + the sorted particle ids (GpuParticles.sorted_ids, src/solver/particle3d.rs:178-180)
 * of the last substep. sorted_ids may be NULL. */
wgs_status wgs_read_blocks(wgs_data *data, wgs_block_record *out, size_t capacity, size_t *count, uint32_t *sorted_ids);
/* GpuTimestamps read-back (src_testbed/step.rs:219-251): ms per pass summed over the substeps of the
 * last wgs_step(.., timestamps=1) call. */
wgs_status wgs_read_timings(wgs_data *data, float ms[WGS_NUM_PASSES]);
/* The cost of one timing mark (a HIP event is a barrier packet of its own): the average distance of two marks
 * recorded back to back in the same timestamped substeps. Every pass time of wgs_read_timings includes one; a pass
 * with K launches between its marks took (time - overhead) of kernel time. */
wgs_status wgs_read_timing_overhead(wgs_data *data, float *ms_per_mark);
wgs_status wgs_get_stats(wgs_data *data, wgs_stats *out);
/* Per-material constants are per-PARTICLE data in the reference (GpuModels, src/models/mod.rs:12-50; init_volume and
 * mass in ParticleDynamics), re-read by every pass. When every particle of a simulation has the same (mass,
 * init_volume, lambda, mu) the step keeps them as kernel arguments instead (32 bytes per particle and substep less
 * through HBM; results are bit-identical). wgs_data_create detects this by itself; on SHARDED data a rank only sees
 * its own particles, so the caller asserts it — on every rank, before the first step — with this call. 3D only
 * (a no-op in the 2D library). */
wgs_status wgs_set_uniform_material(wgs_data *data, float mass, float init_volume, float lambda, float mu);
/* The reference sizes the sparse grid once and has a stub where it should grow it ("TODO: resize the hashmap and
 * retry", src/grid/grid.rs:43-45,116-117); blocks beyond the capacity are dropped silently
 * (src/grid/grid.wgsl:126-128). Here, by default, the block capacity DOUBLES whenever a wgs_step / wgs_sharded_step
 * call finds that the previous call ended with more than half of it active (the check reads counters left in pinned
 * host memory: no synchronisation; the growth itself drains the stream once). Particle state is untouched: the next
 * substep rebuilds the table. enabled = 0 restores the fixed capacity; WGS_ERR_GRID_OVERFLOW remains for growth that
 * outruns the check (more than half a capacity of new blocks inside one call). */
wgs_status wgs_set_grid_growth(wgs_data *data, int32_t enabled);
/* Domain walls. NEW: the reference builds every container from CPIC collider cuboids; a wall is the cheap form for a boundary that
 * never moves and is axis-aligned — a boundary condition on the grid, one short launch between the grid update and G2P, no collider
 * slot. A face is a half-space of grid NODES in world cell coordinates, the integers wgs_read_grid reports in wgs_node_record.cell:
 * the low face of axis k holds every node with cell[k] <= plane, the high face every node with cell[k] >= plane. Planes are
 * integers on purpose: membership is exact, independent of the cell width, and the same on host and device.
 * A node inside a face, after the grid update (velocity v, mass untouched), with vn = the component INTO the wall (-v[k] on a low
 * face, +v[k] on a high one) and vt = the other components:
 *   WGS_WALL_STICKY    v = 0 in every component;
 *   WGS_WALL_SLIP      v[k] = 0, then vt *= max(0, 1 - friction * |vn| / |vt|) — Coulomb friction in velocity form; |vt| == 0
 *                      leaves vt alone, friction == 0 leaves vt bit for bit;
 *   WGS_WALL_SEPARATE  like WGS_WALL_SLIP where vn > 0, otherwise the node is left bit for bit.
 * A node inside several faces (edges, corners) takes them one after the other on the running value, in the order of the array:
 * axis 0 low, axis 0 high, axis 1 low, axis 1 high[, axis 2 low, axis 2 high].
 * walls[2*k] = low face of axis k, walls[2*k+1] = its high face, 2 * WGS_DIM entries; walls == NULL removes all walls. Stream-ordered
 * like the other setters: the substeps enqueued after the call use it. The walls travel as a kernel argument: no device memory
 * (wgs_stats.device_bytes does not change), no upload; data without walls launches exactly what it launched before.
 * wgs_read_grid, wgs_sample_grid, wgs_read_grid_window and the WGS_DIAG_GRID sums see the velocities AFTER the walls; the time of
 * the launch is reported under WGS_PASS_GRID_UPDATE. Colliders and walls may be used together: the walls act on the node values
 * the CPIC paths read.
 * Containment: a particle with x[k] < (plane - 0.5) h has its whole stencil inside the low face, so what it gathers from a sticky,
 * slip or separating face has no velocity into the wall; the speed cap h / dt moves a particle at most h per substep. Every
 * particle therefore keeps (low.plane - 1.5) h <= x[k] <= (high.plane + 1.5) h — a bound for fast material, not the rest
 * position. Measured (notes/round_26.md: a column settled for 6 000 substeps in a box of walls, h = 1): the lowest particles rest
 * 0.06 h (Tait fluid, slip) to 0.38 h (Tait fluid, sticky) and 0.27-0.49 h (neo-Hookean) on the INNER side of the low plane, none
 * beyond it. So a scene that wants material to rest on a surface puts the plane on it (Wall.low / Wall.high of the Python mirror),
 * and a scene that must never see a particle beyond a surface — a render box, a sensor — places the plane a cell and a half inside
 * that surface: the surface it is guaranteed lies a cell and a half outside the plane it sets.
 * Errors (nothing is changed): type > 3, a friction that is not finite or is negative, both faces of an axis set with
 * low.plane >= high.plane, NULL data / NULL out -> WGS_ERR_INVALID_ARGUMENT; sharded data (wgs_data_create_sharded) ->
 * WGS_ERR_UNSUPPORTED, like wgs_sample_grid. */
enum { WGS_WALL_NONE = 0, WGS_WALL_STICKY = 1, WGS_WALL_SLIP = 2, WGS_WALL_SEPARATE = 3 };
typedef struct { uint32_t type; float friction; int32_t plane; } wgs_wall;   /* 12 bytes, both dimensions */
wgs_status wgs_set_domain_walls(wgs_data *data, const wgs_wall *walls /* 2*WGS_DIM, or NULL */);
/* What wgs_set_domain_walls last took (2 * WGS_DIM entries); all WGS_WALL_NONE when none is set. */
wgs_status wgs_get_domain_walls(wgs_data *data, wgs_wall *out);
/* Snow plasticity. NEW: the reference's only plastic material is Drucker-Prager sand. WGS_PLASTICITY_SNOW is the singular-value clamp
 * with hardening of Stomakhin et al. 2013, on the corotated stress. One rule per wgs_data (default WGS_PLASTICITY_DRUCKER_PRAGER): it
 * says which projection the plastic particle update applies and how the six slots of a particle's wgs_drucker_prager are read.
 * A particle is a snow particle under the gate that sends it into the Drucker-Prager projection otherwise: phase == 0 (from the start,
 * or broken in this substep) and plasticity.lambda != 0. Its slots then mean
 *     h0 = theta_c  critical compression      h1 = theta_s  critical stretch      h2 = xi  hardening coefficient
 *     h3 = the cap on the hardening exponent  lambda = the switch alone (non-zero: on)     mu = unused
 * (the struct is not touched: WGS_MODEL_FLUID reinterprets wgs_elastic_coefficients the same way). Per snow particle and substep, all
 * in fp32, with s_k the signed singular values of the trial matrix F + (G dt) F (U, V proper rotations, the sign on the smallest),
 * Jp = wgs_plastic_state.plastic_deformation_gradient_det and lambda, mu = the particle's own wgs_elastic_coefficients:
 *     s^_k = min(max(s_k, 1 - theta_c), 1 + theta_s)
 *     Jp'  = Jp * prod |s_k| / prod s^_k
 *     F_E  = U diag(s^) V^T                          stored in def_grad
 *     hf   = exp(min(xi * (1 - Jp'), h3))
 *     tau  = the corotated stress of F_E with lambda * hf, mu * hf
 * lambda, mu are stored unchanged (hf is never stored); plastic_hardening and log_vol_gain are written back bit for bit. hf is taken
 * of the UPDATED Jp on purpose: whoever reads the stored state recomputes the very coefficients the step applied. A particle that
 * does not pass the gate is advanced exactly as without the switch. An inverted or vanished singular value comes back to
 * 1 - theta_c; Jp' >= 0 always, and 0 where a singular value vanished.
 * Preconditions on the parameters, the caller's: 0 <= theta_c < 1, theta_s >= 0, xi and h3 finite (the Python mirror models.Snow
 * checks them). They enter arithmetic only: no value makes a kernel read or write outside its arrays.
 * What follows the rule: wgs_read_particle_fields[_device] evaluate the stress of a snow particle with lambda * hf, mu * hf, hf of the
 * stored Jp (wgs_particle_field.model stays WGS_MODEL_COROTATED); WGS_SUM_ELASTIC takes Psi with the same coefficients
 * (max_wave_speed keeps the stored ones). The state digest, wgs_read_particles and wgs_set_plastic_state are unchanged, so
 * wgs_read_particles (+ plastic state) -> wgs_data_create -> wgs_set_plastic_state -> wgs_set_plasticity_model(WGS_PLASTICITY_SNOW)
 * restarts a run bit for bit.
 * Stream-ordered like the other setters: the substeps and read-outs enqueued after the call use it; no device memory, no launch.
 * WGS_PLASTICITY_DRUCKER_PRAGER, or WGS_PLASTICITY_SNOW on data whose step carries no plastic state, launches exactly what was
 * launched before. Errors (nothing is changed): an unknown kind, NULL data / NULL out -> WGS_ERR_INVALID_ARGUMENT; sharded data
 * (wgs_data_create_sharded: the arrivals' kernel has no snow variant) -> WGS_ERR_UNSUPPORTED from the setter, like wgs_set_domain_walls
 * (the getter answers WGS_PLASTICITY_DRUCKER_PRAGER there); WGS_PLASTICITY_SNOW while the data's model is not WGS_MODEL_COROTATED or
 * a table of per-particle models is set -> WGS_ERR_UNSUPPORTED; and while WGS_PLASTICITY_SNOW is set,
 * wgs_set_constitutive_model(any other model) -> WGS_ERR_UNSUPPORTED. */
enum { WGS_PLASTICITY_DRUCKER_PRAGER = 0, WGS_PLASTICITY_SNOW = 1 };
wgs_status wgs_set_plasticity_model(wgs_data *data, int32_t kind);
wgs_status wgs_get_plasticity_model(wgs_data *data, int32_t *out);
/* Force fields (uniform, radial, vortex and drag zones on the grid nodes): an extension header of their own — wgs_force_field,
 * the force and region kinds, the limit of eight fields per data, wgs_set_force_fields / wgs_get_force_fields and the rule. */
#include "wgsparkl_hip_forces.h"
/* Particles added at run time (a reserved particle capacity, batches appended by the caller, emitters fired by the library): an
 * extension header of their own — wgs_data_create_reserved, wgs_get_particle_capacity, wgs_add_particles, wgs_emitter and its
 * setter, getter and counters, the lattice and the schedule. */
#include "wgsparkl_hip_emit.h"
/* Particles removed at run time (a mask of the caller's, regions evaluated on the device, sinks the library evaluates on a schedule):
 * an extension header of their own — wgs_remove_particles[_device], wgs_remove_particles_in, wgs_sink and its setter, getter and
 * counters, the membership rule, the renumbering and the schedule. */
#include "wgsparkl_hip_remove.h"
/* Environment (read once per wgs_data_create; developer switches, none of them changes a result): WGS_DEBUG = bit mask of
 * launch-SHAPE choices (two launches instead of one paired launch, the general binning pass on every substep, the grid
 * update and the message packing as launches of their own instead of workgroups of the P2G launch, ...) and
 * WGS_REHASH_PERIOD = substeps between unconditional rebuilds of the block table — used by the A/B tools and by the tests
 * that assert those shapes are bit-identical; WGS_TRACE drains the stream at every pass boundary and says so on stderr.
 * bench.py refuses to run with WGS_DEBUG / WGS_REHASH_PERIOD set. Switches that DO change results (ablations for timing
 * experiments) exist only in builds with -DWGS_ABLATE, which wgs_build_info() names and bench.py refuses. */
/* TEST HOOK (not part of the drop-in surface): runs the device-side exclusive scan that replaces WgPrefixSum
 * (src/grid/prefix_sum.rs:17-152, prefix_sum.wgsl:11-93) on caller data, so that the reference's own scan test
 * vectors (src/grid/prefix_sum.rs:183-229) can be put through the HIP code: out[i] = sum of values[0..i), *total
 * (may be NULL) = sum of all. Blocking. */
wgs_status wgs_debug_scan(wgs_pipeline *pipeline, const uint32_t *values, uint32_t n, uint32_t *out, uint32_t *total);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU (x-slab domain decomposition). NEW DESIGN: the reference is single-GPU (one wgpu::Device,
 * src/pipeline.rs:176-193; SURVEY.md sections 5 and 8e). One process per GPU owns the particles whose
 * associated block has bx in [block_lo, block_hi) — its core range — and ONE neighbour exchange per substep
 * (wgsparkl_amd/csrc/kernels_shard.h): after P2G both neighbours swap the partial (momentum, mass) sums of the node
 * layers they share, and in the SAME message the records of the particles that left the sender's core range in the
 * previous substep; the old owner still transfers such a particle to the grid in this substep, the new owner runs its
 * G2P + particle update from the message and keeps it. No host synchronisation anywhere inside a substep.
 * `global_ids` are the particles' ids in the global scene (the canonical summation order is by id, so a
 * sharded run reproduces the single-GPU sums). All ranks must pass the same `force_plastic`.
 * The caller replays the reference contract — one call per frame, src_testbed/step.rs:122-128:
 *   rank 0: wgs_comm_get_unique_id(id) -> the host broadcasts the 128 bytes (MPI, torch.distributed, a file ...)
 *   every rank: wgs_comm_create(pipeline, id, rank, world, 0, &comm)      (ncclCommInitRank; rank r talks to r-1, r+1)
 *               wgs_data_create_sharded(...); wgs_shard_attach(data, comm, 0, 0, halo_cap, mig_cap)
 *   per frame:  wgs_sharded_step(pipeline, data, num_substeps); ... wgs_sync(data)
 * RCCL point-to-point is the transport, bound at run time with dlopen("librccl.so.1"): the library has no link-time
 * dependency on RCCL and single-GPU users never load it. */
wgs_status wgs_data_create_sharded(wgs_pipeline *pipeline, const wgs_sim_params *params,
                                   const wgs_particle *particles, size_t num_particles, const uint32_t *global_ids,
                                   const wgs_collider *colliders, size_t num_colliders, float cell_width,
                                   uint32_t grid_capacity, uint32_t particle_capacity, int32_t block_lo,
                                   int32_t block_hi, int32_t force_plastic, wgs_data **out);
/* Sizes of the records a message holds (for choosing the capacities of wgs_shard_attach and reading wgs_shard_export):
 * a halo record = key + the partial sums of ONE x-layer pair of a block (2 * BW^(D-1) nodes); a particle record = the
 * quads of wgsparkl_amd/csrc/layout.h + persistent id + cdf epoch — in uniform-material mode (wgs_set_uniform_material;
 * 3D) the fourth word of its first quad holds F[8] instead of the mass and its F2 quad is not maintained. */
uint32_t wgs_shard_halo_record_bytes(void);
uint32_t wgs_shard_particle_record_bytes(void);
uint32_t wgs_shard_buffer_header_bytes(void);    /* every message / export buffer = header + records */
/* Run this wgs_data on the caller's HIP stream, so that its kernels are ordered with the caller's own work without host
 * synchronisation. The handle does not take ownership; the stream must outlive it. */
wgs_status wgs_set_stream(wgs_data *data, void *hip_stream);
/* full records of every particle this rank holds (read-back of a sharded run; BLOCKING). Between two calls of
 * wgs_sharded_step a rank also holds the particles that left its core range in the last substep: they are handed over
 * with the next substep's message, every particle is held by exactly one rank at any time. */
wgs_status wgs_shard_export(wgs_data *data, void *device_buf, uint32_t capacity_records, uint32_t *count);

#define WGS_COMM_ID_BYTES 128          /* ncclUniqueId */
#define WGS_COMM_SELF_NEIGHBOURS 1     /* flag: the rank is its own lower and upper neighbour (one-GPU timing proxy of an interior rank) */
typedef struct wgs_comm wgs_comm;
wgs_status wgs_comm_get_unique_id(uint8_t id[WGS_COMM_ID_BYTES]);
wgs_status wgs_comm_create(wgs_pipeline *pipeline, const uint8_t id[WGS_COMM_ID_BYTES], int32_t rank, int32_t world,
                           int32_t flags, wgs_comm **out);
/* Every wgs_data attached to the communicator must have been synchronised (wgs_sync) or destroyed before. */
void wgs_comm_destroy(wgs_comm *comm);
/* Allocates the message buffers of this slab (one outgoing, one incoming per neighbour; owned by the wgs_data, fixed
 * capacity, sent whole: no size handshake; an overflow is reported by the next wgs_sync). Call before the first step.
 * With a communicator the neighbours are the ranks next to comm's (has_lower / has_upper are ignored); comm == NULL = a
 * slab of a lockstep group inside one process (wgs_sharded_step_lockstep), or a slab without neighbours.
 * `halo_capacity_records`: halo records per message — about twice the active blocks of a face of the slab (every block
 * of the interface layer sends one x-layer pair, the blocks migrating particles touch a few more);
 * `migrant_capacity`: particles that can cross one face in one substep. A slab with TWO neighbours must be at least
 * 3 blocks wide.
 * What each capacity must cover, exactly (a capacity that is exactly reached is enough and changes no result; one short
 * is reported by the next wgs_sync, and from then on the run is wrong: a pair or a particle was dropped):
 *   halo_capacity_records  the records of ONE message of one substep. The message to the upper neighbour holds, for
 *                          every ACTIVE block (a block that holds a particle of this slab, guests included, or is the
 *                          "+" neighbour of one) of block layer block_hi, its first x-layer pair always and every other
 *                          pair with a non-zero node, and for layer block_hi + 1 its first pair when non-zero; the message
 *                          to the lower neighbour likewise the first pair of every active block of layer block_lo and
 *                          every non-zero pair of layer block_lo - 1. The table is never cleared: only the records of
 *                          the current substep count. The smallest non-empty message holds 2^(D-1) records.
 *   migrant_capacity       the particles that leave through ONE face in ONE substep (each face has its own area).
 *   particle_capacity      (wgs_data_create_sharded) the residents of a substep INCLUDING the guests — the particles that
 *                          left the core range in the previous substep and are handed over in this one — plus the
 *                          particles that arrive in the same substep: the arrivals are written behind all residents
 *                          before the guests' slots are given up.
 *   the leavers' list      is not the caller's to size: max(4096, particle_capacity / 16) particles can leave a slab's
 *                          core range (through both faces together) in one substep.
 * Two-way coupled (dynamic) bodies: every rank accumulates the fixed-point impulses of its own
 * particles (src/solver/p2g.wgsl:142-155) and the 16 x 8 int32 sums are all-reduced before integrate_bodies
 * (src/solver/rigid_impulses.wgsl:94-137) — integers, so the result does not depend on the order. */
wgs_status wgs_shard_attach(wgs_data *data, wgs_comm *comm, int32_t has_lower, int32_t has_upper,
                            uint32_t halo_capacity_records, uint32_t migrant_capacity);
/* `num_substeps` whole substeps of this rank's slab, asynchronous (MpmPipeline::queue_step + encode x N + submit,
 * src/pipeline.rs:195-281, for one slab of the decomposition). Every rank must call it with the same count. */
wgs_status wgs_sharded_step(wgs_pipeline *pipeline, wgs_data *data, uint32_t num_substeps);
/* The same phases for `num_slabs` slabs that live in ONE process on ONE device (passed in x order, attached with
 * comm == NULL), device-to-device copies as the transport: decomposition tests on a single GPU. For the duration of
 * the call the group's work is ordered on slab 0's stream; afterwards every slab's own stream waits for it. */
wgs_status wgs_sharded_step_lockstep(wgs_pipeline *pipeline, wgs_data **slabs, uint32_t num_slabs, uint32_t num_substeps);

/* ---------------------------------------------------------------------------------------------
 * Device-side diagnostics. NEW: the reference has no counterpart (its host can only map `positions`,
 * src/solver/particle3d.rs:197-201; nothing in src/pipeline.rs:195-281 reduces anything). Conserved sums, bounds and a state digest of
 * the state after the last enqueued substep, reduced on the device: no particle crosses PCIe. Per-particle values are the canonical ones
 * wgs_read_particles returns (the uniform-material / uniform-plasticity layouts are undone first). Everything is ORDER-INDEPENDENT by
 * construction — storage order, launch shapes, the side of the ping-pong, rebuilds, evictions and restarts do not change one bit of the
 * result — because nothing on the way is a floating-point addition: sums are 64-bit INTEGER sums of fixed-point terms, bounds are integer
 * maxima / minima of ordered bit patterns, the digest is a sum modulo 2^64.
 *
 * what = OR of WGS_DIAG_*:
 *   PARTICLES  counts, bounds, and every particle sum but WGS_SUM_ELASTIC (a pure streaming pass, twice);
 *   ENERGY     adds WGS_SUM_ELASTIC (a symmetric eigenvalue problem per particle, in fp64); implies PARTICLES;
 *   GRID       the three grid sums, over the nodes of the blocks active in the last substep, as wgs_read_grid reports them
 *              (velocity after the grid update, mass; x_i = cell * h); all zero before the first substep;
 *   DIGEST     digest[2] (and the counts).
 * Fields that were not asked for are zero; `what` echoes the bits that were computed, `model` the constitutive model.
 *
 * Particles. Slots whose particle now lives on a neighbouring rank (sharded data) are skipped. A particle with a non-finite position,
 * velocity, affine matrix, deformation gradient, mass, init_volume, lambda or mu is counted in num_nonfinite and left out of every sum
 * and bound (it is still in num_particles and in the digest).
 *
 * Terms (fp64, from the fp32 state; a product of two fp32 values is exact there). m = mass, x = position, v = velocity, F = def_grad,
 * A = `affine` AS STORED, V0 = init_volume, h = cell width, g = gravity, D = h^2/4 (inv_d = 4/h^2, src/grid/kernel.wgsl). NOTE on A: the
 * particle update stores A = m * grad v - tau * V0 * inv_d * dt (src/solver/particle_update.wgsl:129-132), and P2G transfers
 * w * (A * (x_i - x) + m v) (src/solver/p2g.wgsl:176-236): A already carries the mass, and the velocity gradient it stands for is C = A / m.
 *   WGS_SUM_MASS              m
 *   WGS_SUM_MOMENTUM + k      m * v_k
 *   WGS_SUM_ANGULAR + k       m * (x cross v)_k + D * axial(A - A^T)_k   — about the origin; what P2G puts on the grid, exactly: sum_i w_i
 *                             (x_i - x)(x_i - x)^T = D * I for the quadratic kernel. axial(A - A^T) = (A_zy - A_yz, A_xz - A_zx, A_yx - A_xy);
 *                             tau is symmetric, so this is m * D * axial(C - C^T) of the velocity gradient. 2D: the z component only, in [+0].
 *   WGS_SUM_MASS_MOMENT + k   m * x_k
 *   WGS_SUM_KINETIC           m * |v|^2 / 2
 *   WGS_SUM_KINETIC_AFFINE    D * |A|_F^2 / (2 m)  = m * D * |C|_F^2 / 2 with C = A / m (0 where m == 0)
 *   WGS_SUM_GRAVITY_POTENTIAL -m * (g . x)
 *   WGS_SUM_ELASTIC           V0 * Psi(F), Psi = the energy whose derivative is the Kirchhoff stress the step applies, tau = (dPsi/dF) F^T,
 *                             under the model of wgs_set_constitutive_model, with the particle's own lambda, mu (F of a Drucker-Prager
 *                             particle is its elastic part):
 *                               corotated   (src/models/linear_elasticity.wgsl:28-41)      Psi = mu * sum_i (s_i - 1)^2 + lambda / 2 * (J - 1)^2,
 *                               neo-Hookean (src/models/neo_hookean_elasticity.wgsl:14-25) Psi = mu / 2 * (tr F^T F - d) - mu * ln J + lambda / 2 * ln^2 J,
 *                                           J = max(det F, 1e-10) as there.
 *                               fluid       (WGS_MODEL_FLUID; F = diag(J, 1[, 1]))          Psi = lambda / gamma * (Jc^(1-gamma) / (gamma - 1) + Jc - gamma / (gamma - 1)),
 *                                           Jc = max(J, 1e-10): dPsi/dJ = -p, Psi(1) = 0. Viscous dissipation is not an energy and has no sum.
 *                             s_i = signed singular values (proper rotations, the sign of det F on the smallest). Evaluated through
 *                             G = F - I and E = G + G^T + G^T G = F^T F - I: s_i - 1 = e_i / (s_i + 1) for the eigenvalues e_i of E (fp64
 *                             cyclic Jacobi; the fp32 SVD of the step would lose (s_i - 1)^2 near the rest state), det F - 1 from the invariants of G.
 *   WGS_SUM_GRID_MASS         m_i
 *   WGS_SUM_GRID_MOMENTUM + k m_i * v_i,k
 *   WGS_SUM_GRID_ANGULAR + k  m_i * (x_i cross v_i)_k,  x_i = cell * h  (2D: [+0])
 *
 * Reproducible accumulation. value == ldexp(fixed, exponent): `fixed` is the sum over particles (nodes) of rint(term * 2^-exponent) as a
 * signed 64-bit integer (the reference's own device for its impulses, src/solver/p2g.wgsl:142-155, fixed point x 1e5 — with a scale that is
 * chosen, not assumed). The components of a vector sum share one exponent:
 *     exponent = b + nbits(N) - 62,   clamped to [-1000, 1000]
 *   b        = the binary exponent of the largest |term| of the sum (all components) as a first pass finds it, in fp64: 2^(b-1) <= max < 2^b
 *              (frexp); b = -200 when every term is zero;
 *   N        = num_particles for the particle sums, 64 * active blocks for the grid sums; nbits(N) = bits of N, N < 2^nbits(N) (nbits(0) = 0).
 * It is the smallest exponent for which N * 2^b stays below 2^62 * 2^exponent, so `fixed` cannot overflow, and the rounding error of a
 * sum is at most N * 2^(exponent - 1). `fixed` sums of EQUAL exponent, counts and digests of the ranks of a sharded run add exactly;
 * combining the ranks is the caller's task.
 *
 * Bounds (exact maxima / minima over the finite particles; where a value is computed it is computed in fp64 and rounded to fp32 once):
 * aabb of x; max_speed = max |v|_2; max_affine_norm = max |A|_F; min / max det F; max_wave_speed = max sqrt((lambda + 2 mu) * V0 / m)
 * (m > 0); cfl = (max |v|_inf * dt) / h in fp32. No finite particle: aabb_min = min_det_f = +inf, aabb_max = max_det_f = -inf, the rest 0.
 *
 * Digest. digest[0] = sum of H(p), digest[1] = sum of mix(H(p) + 0xd1b54a32d192ed03) over every particle held, modulo 2^64, with
 *     mix(z): z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)     (splitmix64)
 *     H = mix(id + 0x9e3779b97f4a7c15);  for every PAIR of words (w0, w1):  H = mix(H + 0x9e3779b97f4a7c15 + (w0 | w1 << 32))
 * id = the particle's persistent id (the caller's index; the global id on sharded data); the words are the bit patterns of position,
 * velocity, def_grad, affine (matrices column-major), the plastic state (3) and the phase (2) — the fields of wgs_read_particles in
 * that order: 29 words in 3D, 17 in 2D, the last pair completed with a zero word. The cdf is left out (it is stamped by epoch). Data
 * whose step carries no plastic state hashes (1, 1, 0) like wgs_read_particles reports it, and the caller's input phase — except on
 * SHARDED data of that kind, which does not hold the phase per slot: the two phase words are zero there (create the slabs with
 * force_plastic to compare them with a single domain).
 *
 * wgs_read_diagnostics blocks (the struct comes back through pinned memory); wgs_enqueue_diagnostics is stream-ordered, returns at
 * once and leaves the struct at `device_out` (DEVICE memory), for a controller that lives on the device or a later copy. Neither
 * writes simulation state: a step that never calls them launches exactly what it launched before. */
enum { WGS_DIAG_PARTICLES = 1, WGS_DIAG_ENERGY = 2, WGS_DIAG_GRID = 4, WGS_DIAG_DIGEST = 8 };
enum { /* indices into wgs_diagnostics.sum[]; vector sums take three slots in both dimensions */
    WGS_SUM_MASS = 0, WGS_SUM_MOMENTUM = 1, WGS_SUM_ANGULAR = 4, WGS_SUM_MASS_MOMENT = 7,
    WGS_SUM_KINETIC = 10, WGS_SUM_KINETIC_AFFINE = 11, WGS_SUM_ELASTIC = 12, WGS_SUM_GRAVITY_POTENTIAL = 13,
    WGS_SUM_GRID_MASS = 14, WGS_SUM_GRID_MOMENTUM = 15, WGS_SUM_GRID_ANGULAR = 18, WGS_NUM_SUMS = 21
};
typedef struct { int64_t fixed; int32_t exponent; uint32_t reserved; double value; } wgs_fixed_sum;
typedef struct {
    uint64_t num_particles, num_nonfinite;
    wgs_fixed_sum sum[WGS_NUM_SUMS];
    float aabb_min[3], aabb_max[3];           /* 2D: [2] = 0 */
    float max_speed, max_affine_norm, min_det_f, max_det_f, max_wave_speed, cfl;
    uint64_t digest[2];
    uint32_t what, model;
} wgs_diagnostics;
wgs_status wgs_read_diagnostics(wgs_data *data, uint32_t what, wgs_diagnostics *out);
wgs_status wgs_enqueue_diagnostics(wgs_data *data, uint32_t what, wgs_diagnostics *device_out);

/* ---------------------------------------------------------------------------------------------
 * Lagrangian field output. NEW: the reference has no counterpart (its host maps `positions` only; stress never leaves
 * src/solver/particle_update.wgsl). What an MPM user looks at first — the stress a particle carries and how far it is strained — is
 * evaluated on the device from the particle's stored state, without 188 bytes per particle over PCIe, a host SVD and a restatement of
 * the constitutive formulae that would not round like the step.
 *
 * Same stress as the step. `stress` is what the step's own functions return for the stored def_grad and the particle's own lambda, mu:
 * a fresh SVD of the stored F, then the corotated (src/models/linear_elasticity.wgsl:14-41) or neo-Hookean
 * (src/models/neo_hookean_elasticity.wgsl:12-25) Kirchhoff stress, the very device functions the particle update calls. For data
 * without plastic state it is therefore bit for bit the tau the next substep would apply if the velocity gradient were zero. For
 * Drucker-Prager data F is the stored (projected) elastic part; the step reuses the SVD its projection maintained, so the two agree to
 * rounding, not to the bit.
 * Fluid, pressure part only. The stress of a WGS_MODEL_FLUID particle is the fluid update with a zero gradient, -Jc p I (Jc, p: WGS_MODEL_FLUID
 * above). The viscous part Jc mu (G + G^T) needs the velocity gradient, which a particle does not store: take it from
 * wgs_sample_grid at the particle positions (velocity_gradient) where it is wanted.
 * Kirchhoff, not Cauchy. Cauchy stress is stress / volume_ratio; the division is left to the caller because J may be zero or negative for
 * an inverted element.
 * The invariants come from the record: mean_stress and von_mises are fp32 functions of the record's own `stress` in one order — the
 * diagonal summed k = 0 .. DIM-1 and divided by DIM; the deviator's entries squared and summed in storage order, times 3/2, square root
 * (the entries are scaled by the power of two of the largest one first and the root scaled back, which is exact: a stress of 1e20 has
 * no fp32 square).
 *
 * No state is written: a step that never calls these launches exactly what it launched before, and no device memory is kept between
 * calls (wgs_stats.device_bytes does not change). Valid at any time, also before the first substep. Records are in the caller's order
 * (record i = particle i of wgs_data_create), wgs_stats.num_particles of them. wgs_read_particle_fields blocks, like wgs_read_particles;
 * the _device form takes a DEVICE pointer aligned to 16 bytes (2D: 8; whatever hipMalloc returns is), is stream-ordered on the data's
 * stream and returns at once, like wgs_prep_vertex_buffer_device. Sharded data (wgs_data_create_sharded) -> WGS_ERR_UNSUPPORTED, like
 * wgs_get_device_ptrs. A NULL argument, or a device pointer off that alignment -> WGS_ERR_INVALID_ARGUMENT and nothing is written. */
typedef struct {
    float stress[WGS_DIM * WGS_DIM]; /* Kirchhoff stress tau of the particle's stored state, column-major like `affine` */
    float mean_stress;               /* tr(stress) / DIM */
    float von_mises;                 /* sqrt(3/2) * |stress - mean_stress * I|_F, in the library's dimension */
    float volume_ratio;              /* J: mat_det(def_grad) as the step takes it; fluid: def_grad[0] */
    float stretch[WGS_DIM];          /* signed singular values of def_grad from the step's svd, in the order it returns them;
                                        fluid: cbrt(J) (2D: sqrt(J)) in every entry, what wgs_prep_vertex_buffer draws */
    uint32_t model;                  /* the model the stress was evaluated under: 0, 1 or 2 (the particle's own where a table is set) */
} wgs_particle_field;                /* 16 words in 3D, 10 in 2D */
/* out: n records, caller's order. */
wgs_status wgs_read_particle_fields(wgs_data *data, wgs_particle_field *out);
wgs_status wgs_read_particle_fields_device(wgs_data *data, wgs_particle_field *device_out);

/* ---------------------------------------------------------------------------------------------
 * Eulerian field output. NEW: the reference has no counterpart (its grid never leaves the device, src/grid/grid.rs; wgs_read_grid above
 * is this library's own host dump of every node). What draws or couples a fluid is a field: here the grid is sampled at arbitrary
 * points, or a dense box of its nodes is copied out, on the device, without a dump of every node over PCIe.
 *
 * The grid is the one wgs_read_grid reports: the nodes of the blocks active in the last executed substep, velocity after the grid update
 * and node mass. EVERY OTHER node counts as velocity 0, mass 0: blocks still in the table but not active in that substep, evicted
 * blocks, blocks outside the packed key range, and everything before the first substep.
 *
 * A sample at x uses the step's own stencil: per axis cell = round(x / h) - 1 (src/solver/particle3d.wgsl:41-49, bit for bit),
 * ref = cell * h - x, the quadratic B-spline weights w of -ref / h (src/grid/kernel.wgsl:60-66), x_i - x = ref + shift * h over the 3^D
 * nodes cell + shift, inv_d = 4 / h^2. velocity and velocity_gradient are what G2P gives a particle at x (src/solver/g2p.wgsl:150-218)
 * before the speed cap and before any CPIC projection: colliders play no part in a sample. One thread sums one sample in one fixed
 * order — the tensor-product order of the step's G2P, x, then y, then z —, so a record depends on its point and the grid only: not on n,
 * not on the order of the points, not on the launch shape.
 * A point with a non-finite coordinate, or whose stencil reaches a block outside the packed key range (src/grid/grid.wgsl:88-95), gives
 * an all-zero record with active_nodes = 0; no input makes a kernel read outside its arrays.
 *
 * n == 0 is WGS_OK and writes nothing. Sharded data (wgs_data_create_sharded) -> WGS_ERR_UNSUPPORTED, like wgs_get_device_ptrs.
 * wgs_sample_grid and wgs_read_grid_window block, like wgs_read_grid; the _device forms take DEVICE pointers, are stream-ordered on the
 * data's stream and return at once, like wgs_prep_vertex_buffer_device. None of the four writes simulation state: a step that never
 * calls them launches exactly what it launched before.
 *
 * A window: `out` holds dims[0] * ... * dims[DIM-1] nodes of DIM + 1 floats each — velocity, then mass; in 3D one float4 —, node
 * (i, j[, k]) of the window = world cell lo + (i, j[, k]) at index i + dims[0] * (j + dims[1] * k). The values are the raw node values of
 * wgs_read_grid, bit for bit; nodes outside the active blocks are +0. Every dims[k] >= 1 and the product of dims below 2^31, else
 * WGS_ERR_INVALID_ARGUMENT and nothing is written. A window partly or wholly outside the key range is allowed and reads zeros there. */
typedef struct {
    float velocity[WGS_DIM];                     /* sum_i w_i v_i */
    float velocity_gradient[WGS_DIM * WGS_DIM];  /* inv_d * sum_i w_i v_i (x_i - x)^T, column-major like `affine` */
    float density;                               /* sum_i w_i m_i / h^DIM */
    uint32_t active_nodes;                       /* stencil nodes that lie in an active block, 0 .. 3^DIM */
} wgs_grid_sample;                               /* 14 words in 3D, 8 in 2D */
/* points: n * DIM floats; out: n records. */
wgs_status wgs_sample_grid(wgs_data *data, const float *points, size_t n, wgs_grid_sample *out);
wgs_status wgs_sample_grid_device(wgs_data *data, const float *device_points, size_t n, wgs_grid_sample *device_out);
/* lo: DIM cell coordinates; dims: DIM extents. */
wgs_status wgs_read_grid_window(wgs_data *data, const int32_t *lo, const uint32_t *dims, float *out);
wgs_status wgs_read_grid_window_device(wgs_data *data, const int32_t *lo, const uint32_t *dims, float *device_out);

#ifdef __cplusplus
}
#endif
#endif /* WGSPARKL_HIP_H */
