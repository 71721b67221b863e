// host_state.h — what every other part of capi.hip builds on: error reporting (fail, HIP_TRY, WGS_TRY), the handle
// structs behind the C ABI, and the owners of everything the HIP runtime hands out. The calls that make or end a resource
// appear in this file only:
//   hipMalloc / hipFree                      DeviceMemory (lives as long as a wgs_data, or until its group is released) and
//                                            Scratch (lives for one call)
//   hipHostMalloc / hipHostFree              Pinned
//   hipEventCreate* / hipEventDestroy        Event, and Events (the block of timing marks: all of them or none)
//   hipStreamCreate* / hipStreamDestroy      DataStream (the data's stream, its own or the caller's)
// Each owner ends what it made when it goes out of scope, whichever way that happens; ScopeExit does the same for an
// action. No kernel and no entry point belongs here.
#pragma once

namespace {

constexpr int D = WGS_DIM;
constexpr int DD = D * D;
using P = Pl<D>;

#define WGS_STR2(x) #x
#define WGS_STR(x) WGS_STR2(x)

thread_local std::string g_last_error;

wgs_status fail(wgs_status code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// Both return from the ENCLOSING function: not for destructors, not for lambdas that clean up.
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(WGS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
    } while (0)
#define WGS_TRY(expr)                          \
    do {                                       \
        const wgs_status _st = (expr);         \
        if (_st != WGS_OK) return _st;         \
    } while (0)

// An action for the end of a scope, whichever way it ends: ScopeExit guard{[&] { ... }};
template <typename F> struct ScopeExit {
    F at_exit;
    ~ScopeExit() { at_exit(); }
};
template <typename F> ScopeExit(F) -> ScopeExit<F>;

// Pinned host memory.
template <typename T> class Pinned {
    T *ptr = nullptr;

public:
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    Pinned &operator=(Pinned &&o) noexcept {
        std::swap(ptr, o.ptr);
        return *this;
    }
    ~Pinned() {
        if (ptr) hipHostFree(ptr);
    }
    wgs_status alloc(size_t count) {
        HIP_TRY(hipHostMalloc((void **)&ptr, sizeof(T) * count, hipHostMallocDefault));
        return WGS_OK;
    }
    T *get() const { return ptr; }
    T &operator[](size_t i) const { return ptr[i]; }
    explicit operator bool() const { return ptr != nullptr; }
};

// One event.
class Event {
    hipEvent_t ev = nullptr;

public:
    Event() = default;
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event &operator=(Event &&o) noexcept {
        std::swap(ev, o.ev);
        return *this;
    }
    ~Event() {
        if (ev) hipEventDestroy(ev);
    }
    wgs_status create(unsigned flags) {
        HIP_TRY(hipEventCreateWithFlags(&ev, flags));
        return WGS_OK;
    }
    operator hipEvent_t() const { return ev; }
};

// The marks of a timestamped wgs_step: created by the first such call, all of them or none.
struct Events {
    static constexpr int MAX_SUBSTEPS = 64;
    static constexpr int MARKS = 11;  // + 2 calibration marks (9, 10) recorded back to back: the cost of a mark itself
    static constexpr int PASS_MARKS = 9;  // boundaries: start, sort, cdf_nodes, cdf_particles, p2g, grid, g2p, g2p near colliders, bodies(end)
    hipEvent_t ev[MAX_SUBSTEPS][MARKS];
    int used = 0;
    bool created = false;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    ~Events() { destroy(created ? MAX_SUBSTEPS * MARKS : 0); }
    wgs_status create() {
        if (created) return WGS_OK;
        for (int k = 0; k < MAX_SUBSTEPS * MARKS; k++) {
            const hipError_t e = hipEventCreateWithFlags(&ev[0][0] + k, hipEventDisableSystemFence);  // timing only: no cache writeback per mark
            if (e != hipSuccess) {
                destroy(k);
                return fail(WGS_ERR_HIP, std::string("hipEventCreateWithFlags (timing marks): ") + hipGetErrorString(e));
            }
        }
        created = true;
        return WGS_OK;
    }

private:
    void destroy(int count) {   // (the first `count` in creation order: row by row)
        for (int k = 0; k < count; k++) hipEventDestroy(*(&ev[0][0] + k));
        created = false;
    }
};

// The stream of one wgs_data: made with it, or the caller's (wgs_set_stream), which is never destroyed here.
class DataStream {
    hipStream_t s = nullptr;
    bool owned = false;

public:
    DataStream() = default;
    DataStream(const DataStream &) = delete;
    DataStream &operator=(const DataStream &) = delete;
    ~DataStream() {
        if (s && owned) hipStreamDestroy(s);
    }
    wgs_status create() {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return fail(WGS_ERR_HIP, "hipStreamCreate failed");
        owned = true;
        return WGS_OK;
    }
    wgs_status borrow(hipStream_t callers) {   // (the caller drained the old one)
        if (s && owned) HIP_TRY(hipStreamDestroy(s));
        s = callers;
        owned = false;
        return WGS_OK;
    }
    // For the length of one call another stream stands in (capi_sharded.inc StreamLoan, which puts the old one back):
    // whose stream it is does not change.
    hipStream_t exchange(hipStream_t other) { return std::exchange(s, other); }
    operator hipStream_t() const { return s; }
};

// Device memory of one wgs_data. Every allocation belongs to a group: `grid` = the arrays sized by the block capacity
// (host_grid.inc alloc_grid lists them, grow_grid replaces the whole group), `rigid` = the samples and vertices of the mesh
// colliders (capi_io.inc rigid_arrays lists them), `models` = the two planes of per-particle models, `fixed` = everything
// else. What a later call replaces goes by release_group.
enum class MemGroup : uint8_t { fixed, grid, old_grid, rigid, models };
class DeviceMemory {
    struct Block { void *ptr; size_t bytes; MemGroup group; };
    std::vector<Block> blocks;
    uint64_t total = 0;

public:
    // `zero_on`: the stream a zero fill is enqueued on (null: left as allocated)
    wgs_status alloc(void **out, size_t bytes, MemGroup group, hipStream_t zero_on, bool zero) {
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, bytes));
        blocks.push_back({p, bytes, group});
        total += bytes;
        *out = p;
        if (zero) HIP_TRY(hipMemsetAsync(p, 0, bytes, zero_on));
        return WGS_OK;
    }
    void release(void *p) {
        if (!p) return;
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].ptr == p) {
                total -= blocks[i].bytes;
                blocks.erase(blocks.begin() + (long)i);
                break;
            }
        hipFree(p);
    }
    void release_group(MemGroup group) {
        for (size_t i = blocks.size(); i-- > 0;)
            if (blocks[i].group == group) release(blocks[i].ptr);
    }
    void release_all() {
        while (!blocks.empty()) release(blocks.back().ptr);
    }
    void regroup(MemGroup from, MemGroup to) {
        for (Block &b : blocks) b.group = b.group == from ? to : b.group;
    }
    uint64_t bytes() const { return total; }   // wgs_stats::device_bytes
};

// Device memory for the length of one call: freed when the scope ends, whichever way it ends.
template <typename T> struct Scratch {
    T *ptr = nullptr;
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { hipFree(ptr); }   // (a null pointer is a no-op)
    wgs_status alloc(size_t count, bool zeroed = false) {   // (zeroed: a synchronous fill, for code that runs on the null stream)
        HIP_TRY(hipMalloc((void **)&ptr, sizeof(T) * (count ? count : 1)));
        if (zeroed) HIP_TRY(hipMemset(ptr, 0, sizeof(T) * (count ? count : 1)));
        return WGS_OK;
    }
};

}  // namespace

namespace { struct DiagAcc; }   // kernels_diag.h

struct wgs_pipeline {
    int device = 0;
    int num_cus = 256;
    hipDeviceProp_t props;
};

// Multi-GPU (capi_sharded.inc): one RCCL communicator of the x-slab chain, and the message buffers of one slab.
struct wgs_comm {
    void *comm = nullptr;
    int rank = 0, world = 1;
    int lower = -1, upper = -1;   // peer ranks, -1 = none
    int device = 0;
};
struct ShardLink {                // device memory owned by the wgs_data: one message per face and direction (kernels_shard.h)
    bool attached = false;
    wgs_comm *comm = nullptr;     // null: lockstep transport (device-to-device copies inside one process)
    bool has_lower = false, has_upper = false;
    uint32_t halo_cap = 0, mig_cap = 0;
    size_t msg_floats = 0;
    float *msg_out[2] = {nullptr, nullptr}, *msg_in[2] = {nullptr, nullptr};   // [lower, upper]
};

struct wgs_data {
    // ---- what the simulation is: set at creation or by a setter
    wgs_pipeline *pipeline = nullptr;
    DataStream stream;
    Dev dev{};
    int side = 0;
    bool plastic = false;
    bool cpic = false;
    uint64_t substeps = 0;
    uint32_t capacity = 0;      // particle slots allocated
    uint32_t *shard_counts = nullptr;  // device scratch for pack kernels
    // by-pid static tables (never reordered)
    float *static_radius = nullptr;
    float *static_dp = nullptr;     // n*6
    float *static_phase = nullptr;  // n*2
    uint32_t *static_flags = nullptr;  // bit0 has_plasticity, bit1 has_phase
    SimParamsDev *sp = nullptr;
    ColliderDev *colliders = nullptr;
    std::vector<ColliderDev> host_colliders;  // what the host last wrote (poses / velocities move on the device)
    std::vector<BodyDev> host_bodies;
    bool bodies_move = false;   // some body has a velocity or a mass: integrate_bodies runs every substep
    uint32_t moving_mask = 0;   // ... which ones (bit per collider; sticky like bodies_move): the blocks out of their reach keep their node cdfs
    bool two_way = false;       // P2G accumulates the bodies' impulses: whenever a body can move (a kinematic body uses
                                // them too: the velocity caps of rigid_impulses.wgsl:112-125 apply once it is pushed)
    bool mesh_cdf = false;      // mesh colliders were set at some point: the grid group holds their accumulators (Dev::mesh_min / mesh_aff)
    SimParamsDev host_sp{};
    bool auto_grow = true;
    uint32_t cdf_generation = 1;        // bumped whenever cached node cdfs / block classes become invalid (kernels_sort.h regroup_block)
    uint32_t rehash_period = REHASH_PERIOD;  // substeps between unconditional table rebuilds (developer override: WGS_REHASH_PERIOD); 0 = none
                                             // but the first substep's: data whose long-inactive blocks are evicted (wgs_data_create decides)
    ShardLink *link = nullptr;          // wgs_shard_attach
    int reduce_impulses = 0;            // sharded two-way coupling: 1 = ncclAllReduce of the body impulses before
                                        // integrate_bodies, 2 = the caller sums them and integrates (lockstep group)
    int32_t **lockstep_imp_ptrs = nullptr;
    uint32_t lockstep_imp_n = 0;
    // diagnostics (kernels_diag.h): accumulators and the result on the device (allocated by the first call, freed with `mem`), pinned host copy
    DiagAcc *diag_acc = nullptr;
    wgs_diagnostics *diag_out = nullptr;
    Pinned<wgs_diagnostics> diag_host;
    // Eulerian field output (capi_probe.inc): the sampler's scratch word per block id (allocated by the first call, freed with `mem`),
    // the capacity it was sized for, and the ticket of the last call
    uint32_t *probe_mark = nullptr;
    uint32_t probe_mark_cap = 0, probe_ticket = 0;
    // domain walls (capi_walls.inc): what wgs_set_domain_walls last took, face by face; `walls_set`: some face is not WGS_WALL_NONE —
    // enqueue_finish then launches k_grid_walls behind the grid update, with these as its argument (no device memory)
    wgs_wall walls[2 * WGS_DIM] = {};
    bool walls_set = false;
    // force fields (capi_forces.inc): what wgs_set_force_fields last took, in its order, and how many; `forces_set`: some entry is not
    // WGS_FORCE_NONE — enqueue_finish then launches k_grid_forces in front of the walls, with these as its argument (no device memory)
    wgs_force_field forces[WGS_MAX_FORCE_FIELDS] = {};
    uint32_t forces_n = 0;
    bool forces_set = false;
    // the plasticity rule (capi_plasticity.inc, wgs_set_plasticity_model): WGS_PLASTICITY_*. A host-side choice of instantiation —
    // launch_g2p, the field read-out and the energy sum pick the snow kernels by it —, not a field of Dev: no kernel that existed
    // gets another argument block
    int32_t plasticity = WGS_PLASTICITY_DRUCKER_PRAGER;
    // emitters (capi_emit.inc): what wgs_set_emitters last took, in its order, and how many; `emit_set`: there is one — wgs_step then asks
    // fire_emitters in front of every substep. Host state like the walls and the fields; the counters are those of wgs_get_emitter_counts
    wgs_emitter emitters[WGS_MAX_EMITTERS] = {};
    uint32_t emit_n = 0;
    bool emit_set = false;
    uint64_t emitted[WGS_MAX_EMITTERS] = {}, emit_skipped[WGS_MAX_EMITTERS] = {};
    // sinks (capi_remove.inc): what wgs_set_sinks last took, in its order, and how many; `sinks_set`: there is one — wgs_step then asks
    // fire_sinks in front of every substep, ahead of the emitters. Host state likewise; the counters are those of wgs_get_sink_counts
    wgs_sink sinks[WGS_MAX_SINKS] = {};
    uint32_t sink_n = 0;
    bool sinks_set = false;
    uint64_t sink_removed[WGS_MAX_SINKS] = {};

    // ---- allocation: every device buffer above and in `dev` (dev_alloc; wgs_data_destroy releases them all)
    DeviceMemory mem;

    // ---- the host's last look at the device counters: written by maintain_grid (the pinned watch) and fetch_counters
    // (wgs_sync and the readers), read by the launch plans
    struct Seen {
        Pinned<uint32_t> watch;        // pinned host copy of the device counters as of the end of the last wgs_step call ...
        Event watch_event;             // ... and the event behind that copy: made together (watch_counters), both or neither
        bool watch_pending = false;
        uint32_t watch_skips = 0;
        uint32_t errors = 0;           // sticky: CTR_ERRORS of every look
        uint32_t nblocks = 0;          // active blocks as last seen by the host, wgs_sync or the pinned watch (0: not yet): sizes the P2G grid
        uint32_t sync_nblocks = 0;     // ... at the last wgs_sync, clamped to the capacity (the readers' count)
        uint32_t nv_hint = 0;          // sharded data: particles this slab holds as the host last saw them (the launch bound is the capacity); picks the G2P chunk count per wave
        uint32_t ncpic = UINT32_MAX;   // near-collider list length at the last wgs_sync (picks the P2G launch shape and G2P's register budget)
        uint32_t nvisit = UINT32_MAX;  // visit-list length at the last wgs_sync (sizes the list half of k_g2p_pair)
        uint32_t movers = 0;           // CTR_MOVERS at the last wgs_sync (cumulative, modulo 2^32)
        uint32_t nphys = 0, nfree = 0, ntomb = 0;   // id high-water mark, free list, table marks at the last wgs_sync (wgs_stats)
        bool force_rehash = false;     // ids three quarters handed out: the next substep rebuilds the table
        bool force_refresh = false;    // the marks of evicted blocks crowd the table: the next substep re-inserts the live blocks into a cleared table (k_table_refresh)
    } seen;

    // ---- the substep being enqueued, and what the last one left behind (host_substep.inc)
    struct Substep {
        // what the last substep left behind: written by enqueue_finish (and grow_grid), consumed by the next substep
        bool prev_sorted = false;   // the current buffer is the sorted output of the previous substep (perm_cell, links valid)
        bool needs_compact = false; // sharded: the last substep ran without its neighbours (wgs_step): the counters of its buffer are still to be set
        bool prebinned = false;     // the last fused G2P binned its output for the coming substep (Dev::bin_next): no k_rebin launch then
        bool bodies_pending = false;   // integrate_bodies of the last substep has not run yet (it rides in the next sort launch)
        // the substep being enqueued: decided ONCE by begin_substep, read by the stages behind it
        bool in_sharded_step = false;  // it belongs to wgs_sharded_step[_lockstep]: guests are dropped, the grid update adds the neighbours' sums
        int ts_slot = -1;           // the row of timing events its marks are recorded in (a timestamped wgs_step), -1: none
        uint32_t epoch = 0;
        bool rehash = false;        // it rebuilds the table of block ids
        bool use_rebin = false;     // its sort bins the particles relative to their old block (k_rebin, or the last G2P did: `binned`)
        bool binned = false;
        bool fused_cdf = false;     // node cdfs and block classes ride in launch 2 of its sort
        bool gu_fused = false;      // its grid update rides in its P2G launch
        bool shard_fused = false;   // sharded substep: the pack waves and the interior blocks' grid update ride in its P2G launch
        bool arrivals = false;      // sharded substep: the particles that arrive with its messages are advanced (k_g2p_arrivals)
    } sub;

    // ---- statistics (wgs_stats): only ever counted up
    struct Stats {
        uint64_t movers_total = 0;     // Seen::movers, accumulated in 64 bits over the host's looks
        uint64_t table_rebuilds = 0;   // substeps that rebuilt the table of block ids
        uint64_t table_refreshes = 0;
        uint32_t grid_grown = 0;       // times the block capacity was doubled
    } stats;

    // ---- timing: the marks of a timestamped wgs_step and what resolve_timings made of them
    struct Timing {
        Events events;
        float ms[WGS_NUM_PASSES] = {0};
        float mark_overhead_ms = 0.f;   // average distance of two adjacent timing marks in the last timestamped step
        std::vector<Event> emit_marks;  // pairs of marks around the emitting launches of a timestamped wgs_step (capi_emit.inc): "grid sort" time
        bool pending = false;
    } timing;
};

namespace {

// Zeroed on the data's stream unless told otherwise (grow_grid drains that stream before it replaces the grid group).
template <typename T> wgs_status dev_alloc(wgs_data *d, T **out, size_t count, MemGroup group = MemGroup::fixed, bool zero = true) {
    return d->mem.alloc(reinterpret_cast<void **>(out), sizeof(T) * (count ? count : 1), group, d->stream, zero);
}

// Copies to the host and waits for it: after this the source may be freed.
wgs_status download(wgs_data *d, void *dst, const void *src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return WGS_OK;
}

// The prologue of every entry point that touches the device: a valid handle (`args_ok`: and valid other pointers), and
// ITS device selected — several wgs_data of several devices may live in one process (capi_sharded.inc).
wgs_status enter(wgs_data *d, bool args_ok = true, const char *what = "NULL argument") {
    if (!d || !args_ok) return fail(WGS_ERR_INVALID_ARGUMENT, what);
    HIP_TRY(hipSetDevice(d->pipeline->device));
    return WGS_OK;
}

int grid_for(const wgs_data *d, int blocks_per_cu) { return d->pipeline->num_cus * blocks_per_cu; }

}  // namespace
