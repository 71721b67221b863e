// wgsparkl_hip.hpp — C++17 host-side mirror of the reference's Rust API for the substep path, header-only, over the C ABI
// of wgsparkl_hip.h (define WGS_DIM = 2 or 3 before including; link libwgsparkl{2,3}d_hip.so).
//
// The reference's host is Rust (src/pipeline.rs, src/solver/particle3d.rs, src/models/mod.rs); this image has no Rust
// toolchain, so the compiled-language host side is C++. Names, argument meaning and error behaviour follow the
// reference's call sites (src/pipeline.rs:98-128,176-200; src_testbed/step.rs:79-132; examples/sand3.rs:28-113):
//
//   reference (Rust)                                           this header
//   ---------------------------------------------------------  -------------------------------------------------------
//   MpmPipeline::new(&device) -> Result<Self, ComposerError>    wgsparkl::MpmPipeline::create(hip_device)   (throws Error)
//   MpmData::new(device, params, &particles, &bodies,           wgsparkl::MpmData::create(pipeline, params, particles,
//                &colliders, cell_width, grid_capacity)                                   colliders, cell_width, grid_capacity)
//   pipeline.queue_step(&mut data, &mut queue, timestamps);     pipeline.queue_step(data, num_substeps, timestamps)
//   for _ in 0..n { queue.encode(..) }; submit                    (records AND submits n substeps; asynchronous)
//   device.poll(Maintain::Wait)                                 data.sync()
//   ParticleDynamics::with_density(radius, density)             wgsparkl::with_density(radius, density)
//   ElasticCoefficients::from_young_modulus(E, nu)              wgsparkl::from_young_modulus(E, nu)
//   DruckerPrager::new(E, nu)                                   wgsparkl::drucker_prager(E, nu)
//   Result / panics                                             wgsparkl::Error (status + wgs_last_error()); no CPU fallback:
//                                                               create() throws WGS_ERR_NO_DEVICE without a HIP device
#ifndef WGSPARKL_HIP_HPP
#define WGSPARKL_HIP_HPP

#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "wgsparkl_hip.h"

namespace wgsparkl {

struct Error : std::runtime_error {
    wgs_status status;
    Error(wgs_status st, const char *what) : std::runtime_error(what ? what : "wgsparkl error"), status(st) {}
};

inline void check(wgs_status st) {
    if (st != WGS_OK) throw Error(st, wgs_last_error());
}

// src/models/mod.rs:52-75 ElasticCoefficients::from_young_modulus / lame_lambda_mu
inline wgs_elastic_coefficients from_young_modulus(float young_modulus, float poisson_ratio) {
    const float d = (1.0f + poisson_ratio) * (1.0f - 2.0f * poisson_ratio);
    return {young_modulus * poisson_ratio / d, young_modulus / (2.0f * (1.0f + poisson_ratio))};
}

// src/models/drucker_prager.rs:17-34 DruckerPrager::new (h0 = 35 deg, h1 = 9 deg, h2 = 0.2, h3 = 10 deg)
inline wgs_drucker_prager drucker_prager(float young_modulus, float poisson_ratio) {
    // (a non-positive modulus keeps the reference's placeholder lambda = mu = -1: "take them from the particle's model")
    const wgs_elastic_coefficients c = young_modulus > 0.0f ? from_young_modulus(young_modulus, poisson_ratio) : wgs_elastic_coefficients{-1.0f, -1.0f};
    const float deg = 3.14159265358979323846f / 180.0f;
    return {35.0f * deg, 9.0f * deg, 0.2f, 10.0f * deg, c.lambda, c.mu};
}

// src/solver/particle3d.rs:28-42 ParticleDynamics::with_density: V0 = (2 r)^dim, m = rho V0, F = I, everything else zero
inline wgs_particle_dynamics with_density(float radius, float density) {
    wgs_particle_dynamics d{};
    for (int k = 0; k < WGS_DIM; k++) d.def_grad[k * WGS_DIM + k] = 1.0f;
    d.init_volume = std::pow(2.0f * radius, (float)WGS_DIM);
    d.init_radius = radius;
    d.mass = density * d.init_volume;
    return d;
}

class MpmData;

// src/pipeline.rs:24-39,176-193 MpmPipeline. Immutable after creation: one pipeline may serve many MpmData.
class MpmPipeline {
  public:
    static MpmPipeline create(int hip_device) {
        // (the structs carry no size field: a library built from another header version is refused here, once — wgsparkl_hip.h)
        if (wgs_abi_version() != WGS_ABI_VERSION) throw Error(WGS_ERR_INVALID_ARGUMENT, "libwgsparkl_hip was built from another version of wgsparkl_hip.h");
        wgs_pipeline *p = nullptr;
        check(wgs_pipeline_create(hip_device, &p));
        return MpmPipeline(p);
    }
    MpmPipeline(MpmPipeline &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    MpmPipeline &operator=(MpmPipeline &&o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    MpmPipeline(const MpmPipeline &) = delete;
    MpmPipeline &operator=(const MpmPipeline &) = delete;
    ~MpmPipeline() { reset(); }

    // queue_step + num_substeps x queue.encode + submit (src/pipeline.rs:195-281, src_testbed/step.rs:122-128,169):
    // asynchronous, stream-ordered
    inline void queue_step(MpmData &data, uint32_t num_substeps, bool add_timestamps = false) const;

    wgs_pipeline *handle() const { return h_; }

  private:
    explicit MpmPipeline(wgs_pipeline *p) : h_(p) {}
    void reset() {
        if (h_) wgs_pipeline_destroy(h_);
        h_ = nullptr;
    }
    wgs_pipeline *h_ = nullptr;
};

// src/pipeline.rs:84-173 MpmData: owns every device buffer of one simulation (RAII like the reference's fields).
class MpmData {
  public:
    // MpmData::new (src/pipeline.rs:98-128): the particle and collider slices are borrowed for the call only
    static MpmData create(const MpmPipeline &pipeline, const wgs_sim_params &params, const std::vector<wgs_particle> &particles,
                          const std::vector<wgs_collider> &colliders, float cell_width, uint32_t grid_capacity) {
        wgs_data *d = nullptr;
        check(wgs_data_create(pipeline.handle(), &params, particles.data(), particles.size(), colliders.data(), colliders.size(),
                              cell_width, grid_capacity, &d));
        return MpmData(d, particles.size(), colliders.size());
    }
    // ... with room for max(particles.size(), particle_capacity) particles in all (wgsparkl_hip_emit.h): add_particles and the emitters fill it
    static MpmData create_reserved(const MpmPipeline &pipeline, const wgs_sim_params &params, const std::vector<wgs_particle> &particles,
                                   const std::vector<wgs_collider> &colliders, float cell_width, uint32_t grid_capacity, uint32_t particle_capacity) {
        wgs_data *d = nullptr;
        check(wgs_data_create_reserved(pipeline.handle(), &params, particles.data(), particles.size(), colliders.data(), colliders.size(),
                                       cell_width, grid_capacity, particle_capacity, &d));
        return MpmData(d, particles.size(), colliders.size());
    }
    MpmData(MpmData &&o) noexcept : h_(std::exchange(o.h_, nullptr)), n_(o.n_), nc_(o.nc_), emitting_(o.emitting_), sinking_(o.sinking_) {}
    MpmData &operator=(MpmData &&o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); n_ = o.n_; nc_ = o.nc_; emitting_ = o.emitting_; sinking_ = o.sinking_; }
        return *this;
    }
    MpmData(const MpmData &) = delete;
    MpmData &operator=(const MpmData &) = delete;
    ~MpmData() { reset(); }

    void set_constitutive_model(int32_t model) { check(wgs_set_constitutive_model(h_, model)); }
    // the Tait exponent of WGS_MODEL_FLUID (default 7; finite and > 1)
    void set_fluid_eos(float gamma) { check(wgs_set_fluid_eos(h_, gamma)); }
    // per-particle constitutive model: one WGS_MODEL_* (0 / 1 / 2) per particle in the caller's order; an empty vector drops the table
    void set_particle_models(const std::vector<uint8_t> &models) {
        if (!models.empty() && models.size() != count()) throw Error(WGS_ERR_INVALID_ARGUMENT, "set_particle_models: one entry per particle");
        check(wgs_set_particle_models(h_, models.empty() ? nullptr : models.data()));
    }
    std::vector<uint8_t> read_particle_models() {
        std::vector<uint8_t> out(count());
        check(wgs_read_particle_models(h_, out.data()));
        return out;
    }
    // domain walls (no reference counterpart): 2 * WGS_DIM faces, [2 k] the low face of axis k (nodes with cell[k] <= plane), [2 k + 1]
    // its high face (cell[k] >= plane); the nodes inside a face have their velocity projected after the grid update (sticky / slip with
    // Coulomb friction / separating). An empty vector removes all walls. Stream-ordered; no device memory.
    void set_domain_walls(const std::vector<wgs_wall> &walls) {
        if (!walls.empty() && walls.size() != 2 * WGS_DIM) throw Error(WGS_ERR_INVALID_ARGUMENT, "set_domain_walls: 2 * WGS_DIM faces");
        check(wgs_set_domain_walls(h_, walls.empty() ? nullptr : walls.data()));
    }
    std::vector<wgs_wall> domain_walls() {
        std::vector<wgs_wall> out(2 * WGS_DIM);
        check(wgs_get_domain_walls(h_, out.data()));
        return out;
    }
    // force fields (no reference counterpart; wgsparkl_hip_forces.h): up to WGS_MAX_FORCE_FIELDS uniform / radial / vortex / drag rules on
    // the grid nodes' velocities, each inside a region, applied in this order behind the grid update and in front of the walls. An empty
    // vector removes them. Stream-ordered; no device memory; not part of a checkpoint.
    void set_force_fields(const std::vector<wgs_force_field> &fields) {
        check(wgs_set_force_fields(h_, fields.empty() ? nullptr : fields.data(), (uint32_t)fields.size()));
    }
    std::vector<wgs_force_field> force_fields() {
        std::vector<wgs_force_field> out(WGS_MAX_FORCE_FIELDS);
        uint32_t n = 0;
        check(wgs_get_force_fields(h_, out.data(), &n));
        out.resize(n);
        return out;
    }
    // particles added at run time (no reference counterpart; wgsparkl_hip_emit.h). add_particles: `particles` behind the residents, with the
    // caller's indices num_particles() ..; every reader includes them at once, the next substep rebuilds the block table. `models`: empty,
    // or one WGS_MODEL_* per new particle (read only while the data carries a per-particle table). Blocking.
    uint32_t particle_capacity() {
        uint32_t cap = 0;
        check(wgs_get_particle_capacity(h_, &cap));
        return cap;
    }
    void add_particles(const std::vector<wgs_particle> &particles, const std::vector<uint8_t> &models = {}) {
        if (!models.empty() && models.size() != particles.size()) throw Error(WGS_ERR_INVALID_ARGUMENT, "add_particles: one model per new particle");
        check(wgs_add_particles(h_, particles.data(), models.empty() ? nullptr : models.data(), particles.size()));
        n_ += particles.size();
    }
    // emitters: up to WGS_MAX_EMITTERS lattice boxes re-emitted every `period` substeps inside step(); an empty vector removes them. The
    // call replaces the whole set and zeroes the counters. Host state of the handle; not part of a checkpoint.
    void set_emitters(const std::vector<wgs_emitter> &emitters) {
        const size_t now = count();
        check(wgs_set_emitters(h_, emitters.empty() ? nullptr : emitters.data(), (uint32_t)emitters.size()));
        emitting_ = !emitters.empty();
        rebase(now);
    }
    std::vector<wgs_emitter> emitters() {
        std::vector<wgs_emitter> out(WGS_MAX_EMITTERS);
        uint32_t n = 0;
        check(wgs_get_emitters(h_, out.data(), &n));
        out.resize(n);
        return out;
    }
    // (particles emitted, batches skipped for lack of room) per emitter slot
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> emitter_counts() const {
        std::vector<uint64_t> emitted(WGS_MAX_EMITTERS), skipped(WGS_MAX_EMITTERS);
        check(wgs_get_emitter_counts(h_, emitted.data(), skipped.data()));
        return {emitted, skipped};
    }
    // particles removed at run time (no reference counterpart; wgsparkl_hip_remove.h). remove_particles: `remove` has one byte per particle
    // in the caller's order, nonzero = remove; the survivors keep their relative order and are renumbered densely, every reader answers
    // them under the new indices at once, the next substep rebuilds the block table. Returns kept_from: the old index of every new
    // index. Blocking (the new particle count is read back). remove_particles_in: the regions of `regions` evaluated on the device, now.
    std::vector<uint32_t> remove_particles(const std::vector<uint8_t> &remove) {
        if (remove.size() != count()) throw Error(WGS_ERR_INVALID_ARGUMENT, "remove_particles: one mask byte per particle");
        if (remove.empty()) return {};
        std::vector<uint32_t> kept_from(remove.size());
        uint32_t removed = 0;
        check(wgs_remove_particles(h_, remove.data(), kept_from.data(), &removed));
        kept_from.resize(remove.size() - removed);
        n_ -= removed;
        return kept_from;
    }
    std::vector<uint32_t> remove_particles_in(const std::vector<wgs_sink> &regions) {
        const size_t now = count();
        std::vector<uint32_t> kept_from(now + 1);
        uint32_t removed = 0;
        check(wgs_remove_particles_in(h_, regions.empty() ? nullptr : regions.data(), (uint32_t)regions.size(), kept_from.data(), &removed));
        kept_from.resize(now - removed);
        n_ -= removed;
        return kept_from;
    }
    // sinks: up to WGS_MAX_SINKS regions evaluated in one pass in front of the substeps their schedule names, ahead of the emitters, inside
    // step() — which waits for the stream there; an empty vector removes them. The call replaces the whole set and zeroes the counters.
    // Host state of the handle; not part of a checkpoint.
    void set_sinks(const std::vector<wgs_sink> &sinks) {
        const size_t now = count();
        check(wgs_set_sinks(h_, sinks.empty() ? nullptr : sinks.data(), (uint32_t)sinks.size()));
        sinking_ = !sinks.empty();
        rebase(now);
    }
    std::vector<wgs_sink> sinks() {
        std::vector<wgs_sink> out(WGS_MAX_SINKS);
        uint32_t n = 0;
        check(wgs_get_sinks(h_, out.data(), &n));
        out.resize(n);
        return out;
    }
    // particles removed per sink slot (a particle in several sinks counts for the first)
    std::vector<uint64_t> sink_counts() const {
        std::vector<uint64_t> removed(WGS_MAX_SINKS);
        check(wgs_get_sink_counts(h_, removed.data()));
        return removed;
    }
    // the plasticity rule (no reference counterpart): WGS_PLASTICITY_DRUCKER_PRAGER (default) or WGS_PLASTICITY_SNOW — singular-value clamp
    // with hardening on the corotated stress; the wgs_drucker_prager slots of a particle then read theta_c, theta_s, xi, exponent cap,
    // switch, unused. Stream-ordered; single-domain data under WGS_MODEL_COROTATED.
    void set_plasticity_model(int32_t kind) { check(wgs_set_plasticity_model(h_, kind)); }
    int32_t plasticity_model() {
        int32_t kind = WGS_PLASTICITY_DRUCKER_PRAGER;
        check(wgs_get_plasticity_model(h_, &kind));
        return kind;
    }
    // device.poll(Maintain::Wait) (src/pipeline.rs:339); also reports device-side sticky errors (grid overflow, key range)
    void sync() { check(wgs_sync(h_)); }
    // the per-frame host -> device writes of src_testbed/step.rs:79-119 and ui.rs:91-104
    void set_sim_params(const wgs_sim_params &p) { check(wgs_set_sim_params(h_, &p)); }
    void set_collider_poses(const std::vector<wgs_pose> &poses) { check(wgs_set_collider_poses(h_, poses.data(), nullptr, poses.size())); }
    void set_body_velocities(const std::vector<wgs_velocity> &vels) { check(wgs_set_body_velocities(h_, vels.data(), vels.size())); }
    void set_body_mass_properties(const std::vector<wgs_mass_properties> &m) { check(wgs_set_body_mass_properties(h_, m.data(), m.size())); }
    // the blocking reads of src_testbed/step.rs:129-132,175-198 (poses) and of the positions buffer (particle3d.rs:197-201)
    std::vector<float> read_positions() {
        std::vector<float> out(count() * WGS_DIM);
        check(wgs_read_positions(h_, out.data()));
        return out;
    }
    // the optional interop view: device pointers to the position quads + ids of the current state (sorted order) and their stream
    wgs_device_ptrs device_ptrs() {
        wgs_device_ptrs v{};
        check(wgs_get_device_ptrs(h_, &v));
        return v;
    }
    std::vector<wgs_particle> read_particles() {
        std::vector<wgs_particle> out(count());
        check(wgs_read_particles(h_, out.data(), nullptr));
        return out;
    }
    std::vector<wgs_pose> read_body_poses() {
        std::vector<wgs_pose> poses(nc_);
        check(wgs_read_body_poses(h_, poses.data(), nullptr, nullptr, nc_));
        return poses;
    }
    // GpuTimestamps (src/pipeline.rs:201-271): milliseconds per named pass of the last timestamped queue_step
    std::vector<float> read_timings() {
        std::vector<float> ms(WGS_NUM_PASSES);
        check(wgs_read_timings(h_, ms.data()));
        return ms;
    }
    wgs_stats stats() {
        wgs_stats s{};
        check(wgs_get_stats(h_, &s));
        return s;
    }
    // reproducible sums, bounds and the state digest of the state after the last enqueued substep, reduced on the device (no
    // reference counterpart); `what` = OR of WGS_DIAG_*. Blocking.
    wgs_diagnostics diagnostics(uint32_t what = WGS_DIAG_PARTICLES) {
        wgs_diagnostics r{};
        check(wgs_read_diagnostics(h_, what, &r));
        return r;
    }
    // Lagrangian field output (no reference counterpart): Kirchhoff stress, its invariants, the volume ratio and the stretches of every
    // particle's stored state, evaluated on the device with the step's own functions; records in the caller's order. The host form
    // blocks; the _device form takes a DEVICE pointer (16-byte aligned), is stream-ordered on the data's stream and returns at once.
    std::vector<wgs_particle_field> particle_fields() {
        std::vector<wgs_particle_field> out(count());
        if (count()) check(wgs_read_particle_fields(h_, out.data()));
        return out;
    }
    void particle_fields_device(wgs_particle_field *device_out) { check(wgs_read_particle_fields_device(h_, device_out)); }
    // Eulerian field output (no reference counterpart): the grid of the last substep sampled at points (n * WGS_DIM floats) and a
    // dense window of its nodes (WGS_DIM + 1 floats per node, x fastest). The host forms block; the _device forms take DEVICE pointers,
    // are stream-ordered on the data's stream and return at once.
    std::vector<wgs_grid_sample> sample_grid(const std::vector<float> &points) {
        std::vector<wgs_grid_sample> out(points.size() / WGS_DIM);
        check(wgs_sample_grid(h_, points.data(), out.size(), out.data()));
        return out;
    }
    void sample_grid_device(const float *device_points, size_t n, wgs_grid_sample *device_out) {
        check(wgs_sample_grid_device(h_, device_points, n, device_out));
    }
    std::vector<float> grid_window(const int32_t (&lo)[WGS_DIM], const uint32_t (&dims)[WGS_DIM]) {
        unsigned long long total = 1;
        for (int k = 0; k < WGS_DIM; k++) total = total < (1ull << 31) ? total * dims[k] : total;
        std::vector<float> out(total != 0 && total < (1ull << 31) ? (size_t)total * (WGS_DIM + 1) : 1);   // (a refused call writes nothing)
        check(wgs_read_grid_window(h_, lo, dims, out.data()));
        return out;
    }
    void grid_window_device(const int32_t (&lo)[WGS_DIM], const uint32_t (&dims)[WGS_DIM], float *device_out) {
        check(wgs_read_grid_window_device(h_, lo, dims, device_out));
    }
    size_t num_particles() const { return count(); }
    wgs_data *handle() const { return h_; }

  private:
    MpmData(wgs_data *d, size_t n, size_t nc) : h_(d), n_(n), nc_(nc) {}
    void reset() {
        if (h_) wgs_data_destroy(h_);
        h_ = nullptr;
    }
    wgs_data *h_ = nullptr;
    // particles the data holds now: created with, added, emitted, less those removed and those the sinks took (host arithmetic on the
    // emitters' and the sinks' counters)
    size_t count() const {
        size_t n = n_;
        if (emitting_)
            for (uint64_t e : emitter_counts().first) n += (size_t)e;
        if (sinking_)
            for (uint64_t r : sink_counts()) n -= (size_t)r;
        return n;
    }
    // after a setter zeroed counters: count() answers `now` again
    void rebase(size_t now) {
        n_ = now;
        n_ += now - count();
    }
    size_t n_ = 0, nc_ = 0;   // n_: without what the current emitters emitted and the current sinks took (modulo 2^64: the sum is what counts)
    bool emitting_ = false, sinking_ = false;
};

inline void MpmPipeline::queue_step(MpmData &data, uint32_t num_substeps, bool add_timestamps) const {
    check(wgs_step(h_, data.handle(), num_substeps, add_timestamps ? 1 : 0));
}

}  // namespace wgsparkl

#endif  // WGSPARKL_HIP_HPP
