// host_sharded.inc — the multi-GPU substep behind the entry points of capi_sharded.inc: the run-time binding of RCCL, the two
// phases of a sharded substep around its one exchange (each a run of the stages of host_substep.inc), and the two transports
// of that exchange.
//
// NEW DESIGN: the reference is single-GPU (one wgpu::Device, src/pipeline.rs:176-193). A caller that replays the
// reference contract — one call per frame, src_testbed/step.rs:122-128 — gets the x-slab decomposition of
// kernels_shard.h through ONE entry point: wgs_sharded_step(pipeline, data, n_substeps) enqueues, per substep,
//   sort .. P2G | pack (interface node sums + guests) | ONE ncclSend/Recv group | grid update (adds the neighbours' sums)
//   + fused G2P + the arrivals' G2P (+ all-reduce of the body impulses + integrate_bodies)
// on the data's stream, with no host synchronisation anywhere. RCCL is bound at run time (dlopen of librccl.so.1: the
// copy the process already loaded — PyTorch-ROCm ships one — or the system's), so the library itself has no link-time
// dependency on it and single-GPU users never load it.
// wgs_sharded_step_lockstep runs the SAME per-phase code for several slabs that live in one process on one device,
// with device-to-device copies as the transport: what the single-GPU parity tests (and a multi-slab run on one GPU) use.
#include <mutex>
#include <dlfcn.h>

namespace {

struct NcclUid { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
enum { NCCL_INT32 = 2, NCCL_FLOAT32 = 7, NCCL_SUM = 0 };

struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(NcclUid *) = nullptr;
    int (*CommInitRank)(void **, int, NcclUid, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string error;
};

Rccl *rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            r.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD);   // the copy this process already uses, if any
            if (r.handle) break;
        }
        for (const char *n : names) {
            if (r.handle) break;
            r.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!r.handle) {
            const char *why = dlerror();
            r.error = std::string("librccl.so.1 not found: ") + (why ? why : "");
            return;
        }
#define RCCL_SYM(field, name)                                                  \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.handle, name));      \
    if (!r.field) r.error = std::string("librccl: missing symbol ") + name;
        RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
        RCCL_SYM(CommInitRank, "ncclCommInitRank")
        RCCL_SYM(CommDestroy, "ncclCommDestroy")
        RCCL_SYM(GroupStart, "ncclGroupStart")
        RCCL_SYM(GroupEnd, "ncclGroupEnd")
        RCCL_SYM(Send, "ncclSend")
        RCCL_SYM(Recv, "ncclRecv")
        RCCL_SYM(AllReduce, "ncclAllReduce")
        RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef RCCL_SYM
    });
    return &r;
}

#define RCCL_TRY(expr)                                                                                              \
    do {                                                                                                            \
        int _rc = (expr);                                                                                           \
        if (_rc != 0)                                                                                               \
            return fail(WGS_ERR_HIP, std::string(#expr) + ": " + (rccl()->GetErrorString ? rccl()->GetErrorString(_rc) : "RCCL error")); \
    } while (0)

// Sum of the fixed-point body impulses of all slabs of a lockstep group (the ncclAllReduce of the RCCL transport):
// integers, so any order gives the same bits.
__global__ void k_impulses_allreduce_local(int32_t **imp, int n) {
    const int t = threadIdx.x;  // 128 = 16 bodies x 8
    int32_t s = 0;
    for (int i = 0; i < n; i++) s += imp[i][t];
    __syncthreads();
    for (int i = 0; i < n; i++) imp[i][t] = s;
}

wgs_status shard_check(wgs_pipeline *pipeline, wgs_data *d) {
    WGS_TRY(enter(d, pipeline != nullptr));
    if (!d->dev.sharded) return fail(WGS_ERR_INVALID_ARGUMENT, "not a sharded wgs_data");
    if (!d->link || !d->link->attached) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_shard_attach has not been called on this wgs_data");
    return WGS_OK;
}

// sharded two-way coupling: every rank holds the impulses of its own particles; all ranks need the sum
wgs_status allreduce_impulses(wgs_data *d) {
    if (!d->link || !d->link->comm) return WGS_OK;
    Rccl *r = rccl();
    RCCL_TRY(r->AllReduce(d->dev.impulses, d->dev.impulses, (size_t)WGS_MAX_COLLIDERS * 8, NCCL_INT32, NCCL_SUM, d->link->comm->comm, d->stream));
    return WGS_OK;
}

// The split form of phase A (DBG_SHARD_SPLIT_LAYERS): the sort, then P2G of the two block layers at each cut —
// the only slabs the outgoing messages are gathered from — with the pack waves behind it, then P2G of every other block with
// the interior's grid update behind it. Same kernels, same sums in the same order as the unsplit form: bit-identical (tested).
wgs_status shard_phase_begin_split(wgs_data *d) {
    WGS_TRY(begin_substep(d, true));
    WGS_TRY(enqueue_sort<D>(d));
    WGS_TRY(enqueue_p2g<D>(d, P2gLayers::boundary));   // + pack waves
    return enqueue_p2g<D>(d, P2gLayers::others);       // + the interior's grid update
}

// phase A: sort .. P2G, then the interface node sums and the guests packed into the outgoing messages
wgs_status shard_phase_begin(wgs_pipeline *p, wgs_data *d) {
    if ((d->dev.dbg & DBG_SHARD_SPLIT_LAYERS) && d->link && (d->link->has_lower || d->link->has_upper) && !(d->dev.dbg & DBG_GU_OWN_LAUNCH))
        return shard_phase_begin_split(d);
    WGS_TRY(begin_substep(d, true));
    WGS_TRY(enqueue_sort<D>(d));
    WGS_TRY(enqueue_p2g<D>(d, P2gLayers::all));
    ShardLink &L = *d->link;
    if (!L.has_lower && !L.has_upper) return WGS_OK;
    if (d->sub.shard_fused) return WGS_OK;   // the pack waves rode in the P2G launch (host_substep.inc begin_substep, plan_p2g)
    const PackWaves pw = pack_waves(d);   // (workgroups of one wave)
    hipLaunchKernelGGL(k_pack_face<D>, dim3(pw.blocks + pw.guests), dim3(64), 0, d->stream, d->dev, d->side, (uint32_t)(d->substeps + 1), pw.blocks);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

// phase B: grid update (which adds the neighbours' partial sums from the inbound messages) + fused G2P + the arrivals' G2P
// (bodies deferred when the caller reduces the impulses itself)
wgs_status shard_phase_end(wgs_pipeline *p, wgs_data *d) { return enqueue_finish<D>(d); }

// one grouped send + receive per neighbour on the data's stream (the two neighbours are distinct peers: each message
// rides its own xGMI link; a rank that is its own neighbour — the one-GPU proxy — matches its sends in order)
wgs_status rccl_exchange(wgs_data *d) {
    const hipStream_t s = d->stream;
    ShardLink &L = *d->link;
    Rccl *r = rccl();
    if (!L.has_lower && !L.has_upper) return WGS_OK;
    RCCL_TRY(r->GroupStart());
    int rc = 0;
    const int peers[2] = {L.comm->lower, L.comm->upper};
    for (int f = 0; f < 2 && rc == 0; f++) {
        if (!(f == 0 ? L.has_lower : L.has_upper)) continue;
        rc = r->Send(L.msg_out[f], L.msg_floats, NCCL_FLOAT32, peers[f], L.comm->comm, s);
        if (rc == 0) rc = r->Recv(L.msg_in[f], L.msg_floats, NCCL_FLOAT32, peers[f], L.comm->comm, s);
    }
    const int rc_end = r->GroupEnd();  // (always closed: a communicator left in group mode would swallow every later call)
    if (rc != 0 || rc_end != 0)
        return fail(WGS_ERR_HIP, std::string("ncclSend / ncclRecv: ") + (r->GetErrorString ? r->GetErrorString(rc != 0 ? rc : rc_end) : "RCCL error"));
    return WGS_OK;
}

}  // namespace
