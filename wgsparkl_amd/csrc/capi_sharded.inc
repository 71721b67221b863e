// capi_sharded.inc — entry points of the multi-GPU decomposition: communicators, wgs_shard_attach, wgs_sharded_step and its
// one-process twin wgs_sharded_step_lockstep (what they enqueue: host_sharded.inc; wgs_shard_export is a reader: capi_io.inc).

namespace {

// The loan of a lockstep group's streams: from here to the end of the scope every slab works on slab 0's stream (the caller
// drained the slabs' own streams first). However the scope ends, the slabs get their own streams back. On the way out of a
// failed call slab 0's stream is drained first: work of every slab may already be queued on it, and a caller that carries
// on — wgs_sync, a read-back, destroy — must not race it. A call that succeeds does not wait: hand_back_waiting.
struct StreamLoan {
    wgs_data **slabs;
    const uint32_t n;
    const hipStream_t s;
    std::vector<hipStream_t> own;
    bool drain = true;
    StreamLoan(wgs_data **slabs_, uint32_t n_) : slabs(slabs_), n(n_), s(slabs_[0]->stream), own(n_) {
        for (uint32_t r = 0; r < n; r++) own[r] = slabs[r]->stream.exchange(s);
    }
    StreamLoan(const StreamLoan &) = delete;
    StreamLoan &operator=(const StreamLoan &) = delete;
    ~StreamLoan() {
        if (drain) hipStreamSynchronize(s);
        for (uint32_t r = 0; r < n; r++) slabs[r]->stream.exchange(own[r]);
    }
    // The end of a call that succeeded: each slab's own stream waits for what the group enqueued (an event), nothing is drained.
    wgs_status hand_back_waiting() {
        Event done;
        WGS_TRY(done.create(hipEventDisableTiming));
        hipError_t e = hipEventRecord(done, s);
        for (uint32_t r = 0; r < n && e == hipSuccess; r++)
            if (own[r] != s) e = hipStreamWaitEvent(own[r], done, 0);
        if (e != hipSuccess) return fail(WGS_ERR_HIP, hipGetErrorString(e));
        drain = false;
        return WGS_OK;
    }
};

}  // namespace

extern "C" {

uint32_t wgs_shard_halo_record_bytes(void) { return (uint32_t)(HaloCfg<D>::REC_F4 * sizeof(float4)); }
uint32_t wgs_shard_particle_record_bytes(void) { return (uint32_t)(particle_record_floats<D>() * sizeof(float)); }
uint32_t wgs_shard_buffer_header_bytes(void) { return 16u; }

wgs_status wgs_comm_get_unique_id(uint8_t id[WGS_COMM_ID_BYTES]) {
    if (!id) return fail(WGS_ERR_INVALID_ARGUMENT, "id is NULL");
    Rccl *r = rccl();
    if (!r->handle || !r->error.empty()) return fail(WGS_ERR_UNSUPPORTED, "RCCL unavailable: " + r->error);
    static_assert(WGS_COMM_ID_BYTES == sizeof(NcclUid), "ncclUniqueId is 128 bytes");
    NcclUid u;
    RCCL_TRY(r->GetUniqueId(&u));
    memcpy(id, u.internal, sizeof(u));
    return WGS_OK;
}

wgs_status wgs_comm_create(wgs_pipeline *pipeline, const uint8_t id[WGS_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t flags,
                           wgs_comm **out) {
    if (!pipeline || !id || !out) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return fail(WGS_ERR_INVALID_ARGUMENT, "rank / world out of range");
    Rccl *r = rccl();
    if (!r->handle || !r->error.empty()) return fail(WGS_ERR_UNSUPPORTED, "RCCL unavailable: " + r->error);
    HIP_TRY(hipSetDevice(pipeline->device));
    NcclUid u;
    memcpy(u.internal, id, sizeof(u));
    std::unique_ptr<wgs_comm> c(new wgs_comm());
    c->rank = rank;
    c->world = world;
    c->device = pipeline->device;
    c->lower = rank > 0 ? rank - 1 : -1;
    c->upper = rank < world - 1 ? rank + 1 : -1;
    if (flags & WGS_COMM_SELF_NEIGHBOURS) c->lower = c->upper = rank;  // one-GPU proxy of an interior rank (timing only)
    const int rc = r->CommInitRank(&c->comm, world, u, rank);
    if (rc != 0) return fail(WGS_ERR_HIP, std::string("ncclCommInitRank: ") + r->GetErrorString(rc));
    *out = c.release();
    return WGS_OK;
}

void wgs_comm_destroy(wgs_comm *comm) {   // (every wgs_data attached to it must be synchronised or destroyed first: see the header)
    if (!comm) return;
    if (comm->comm && rccl()->CommDestroy) rccl()->CommDestroy(comm->comm);
    delete comm;
}

wgs_status wgs_shard_attach(wgs_data *d, wgs_comm *comm, int32_t has_lower, int32_t has_upper, uint32_t halo_capacity_records,
                            uint32_t migrant_capacity) {
    WGS_TRY(enter(d, true, "data is NULL"));
    if (!d->dev.sharded) return fail(WGS_ERR_INVALID_ARGUMENT, "not a sharded wgs_data");
    if (d->link && d->link->attached) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_shard_attach: already attached");
    if (d->substeps != 0) return fail(WGS_ERR_INVALID_ARGUMENT, "wgs_shard_attach: call before the first step");
    if (halo_capacity_records == 0 || migrant_capacity == 0) return fail(WGS_ERR_INVALID_ARGUMENT, "zero message capacity");
    if (comm) {  // the communicator decides who the neighbours are
        if (comm->device != d->pipeline->device) return fail(WGS_ERR_INVALID_ARGUMENT, "communicator of another device");
        has_lower = comm->lower >= 0;
        has_upper = comm->upper >= 0;
    }
    // the block layers the two neighbours' messages touch (lo, lo + 1 and hi - 1, hi) must not overlap
    if (has_lower && has_upper && (int64_t)d->dev.shard_hi - (int64_t)d->dev.shard_lo < 3)
        return fail(WGS_ERR_INVALID_ARGUMENT, "a slab with two neighbours must be at least 3 blocks wide");
    if ((has_lower && d->dev.shard_lo == INT32_MIN) || (has_upper && d->dev.shard_hi == INT32_MAX))
        return fail(WGS_ERR_INVALID_ARGUMENT, "a slab with a neighbour needs a finite block range on that side");
    if (!d->link) d->link = new ShardLink();
    ShardLink &L = *d->link;
    L.comm = comm;
    L.has_lower = has_lower != 0;
    L.has_upper = has_upper != 0;
    L.halo_cap = halo_capacity_records;
    L.mig_cap = migrant_capacity;
    L.msg_floats = msg_floats<D>(L.halo_cap, L.mig_cap);
    for (int f = 0; f < 2; f++) {
        if (!(f == 0 ? L.has_lower : L.has_upper)) continue;
        WGS_TRY(dev_alloc(d, &L.msg_out[f], L.msg_floats));
        WGS_TRY(dev_alloc(d, &L.msg_in[f], L.msg_floats));
    }
    Dev &dev = d->dev;
    dev.shard_has_lo = L.has_lower ? 1u : 0u;
    dev.shard_has_hi = L.has_upper ? 1u : 0u;
    for (int f = 0; f < 2; f++) {
        dev.msg.out[f] = L.msg_out[f];
        dev.msg.in[f] = L.msg_in[f];
    }
    dev.msg.halo_cap = L.halo_cap;
    dev.msg.mig_cap = L.mig_cap;
    L.attached = true;
    return WGS_OK;
}

wgs_status wgs_sharded_step(wgs_pipeline *pipeline, wgs_data *d, uint32_t num_substeps) {
    WGS_TRY(shard_check(pipeline, d));
    wgs_status st = WGS_OK;
    ShardLink &L = *d->link;
    const bool neighbours = L.has_lower || L.has_upper;
    if (neighbours && !L.comm) return fail(WGS_ERR_INVALID_ARGUMENT, "slab has neighbours but no communicator: use wgs_sharded_step_lockstep");
    // body impulses are reduced over ALL ranks (also those without particles near the body) before integrate_bodies
    d->reduce_impulses = (d->two_way && L.comm && L.comm->world > 1) ? 1 : 0;
    if ((st = maintain_grid(d)) != WGS_OK) return st;
    // The exchange is not overlapped with the interior's P2G. Forking it onto a second stream (the boundary layers' P2G, the pack
    // waves and the send / receive there, the rest of P2G on the data's stream) was measured slower on ROCm 7.0 / 7.2, MI355X:
    // every cross-stream dependency cost 15-20 us, more than the 14-16 us RCCL kernel it hid — one rank as its own two
    // neighbours, 1 M slab: 139-145 us serial, 168-175 us forked (520 us with the second stream at a raised priority: every
    // kernel of BOTH queues then took several times its time). The fork was removed; the split of P2G it used remains
    // (shard_phase_begin_split).
    for (uint32_t i = 0; i < num_substeps; i++) {
        if (i > 0 && i % 64u == 0u && ((st = watch_counters(d)) != WGS_OK || (st = maintain_grid(d)) != WGS_OK)) return st;
        if ((st = shard_phase_begin(pipeline, d)) != WGS_OK) return st;
        if (neighbours && (st = rccl_exchange(d)) != WGS_OK) return st;
        if ((st = shard_phase_end(pipeline, d)) != WGS_OK) return st;
    }
    return watch_counters(d);
}

wgs_status wgs_sharded_step_lockstep(wgs_pipeline *pipeline, wgs_data **slabs, uint32_t num_slabs, uint32_t num_substeps) {
    if (!pipeline || !slabs || num_slabs == 0) return fail(WGS_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t r = 0; r < num_slabs; r++) {
        WGS_TRY(shard_check(pipeline, slabs[r]));
        ShardLink &L = *slabs[r]->link;
        if (L.comm) return fail(WGS_ERR_INVALID_ARGUMENT, "lockstep slabs must be attached without a communicator");
        if (L.has_lower != (r > 0) || L.has_upper != (r + 1 < num_slabs))
            return fail(WGS_ERR_INVALID_ARGUMENT, "lockstep slabs must be passed in x order, attached with has_lower / has_upper to match");
        if (L.msg_floats != slabs[0]->link->msg_floats && num_slabs > 1)
            return fail(WGS_ERR_INVALID_ARGUMENT, "all slabs of a lockstep group need the same message capacities");
        if (slabs[r]->pipeline->device != pipeline->device) return fail(WGS_ERR_INVALID_ARGUMENT, "lockstep slabs live on one device");
    }
    bool two_way = false;
    for (uint32_t r = 0; r < num_slabs; r++) two_way = two_way || slabs[r]->two_way;
    if (two_way && num_slabs > 1)
        for (uint32_t r = 0; r < num_slabs; r++)
            if (!slabs[r]->two_way) return fail(WGS_ERR_INVALID_ARGUMENT, "two-way coupling must be enabled on every slab or none");
    HIP_TRY(hipSetDevice(pipeline->device));
    // One stream orders everything FOR THE DURATION OF THIS CALL: every slab's own stream is drained, its work goes to
    // slab 0's stream, and before returning each slab gets its own stream back, made to wait for the group's work (an
    // event): no slab depends on another slab's lifetime afterwards.
    for (uint32_t r = 1; r < num_slabs; r++)
        if (slabs[r]->stream != slabs[0]->stream) HIP_TRY(hipStreamSynchronize(slabs[r]->stream));
    StreamLoan loan(slabs, num_slabs);   // (every return below hands the streams back)
    const hipStream_t s = loan.s;
    int32_t **imp_ptrs = nullptr;
    if (two_way && num_slabs > 1) {
        std::vector<int32_t *> host(num_slabs);
        for (uint32_t r = 0; r < num_slabs; r++) host[r] = slabs[r]->dev.impulses;
        wgs_data *d0 = slabs[0];
        if (!d0->lockstep_imp_ptrs || d0->lockstep_imp_n != num_slabs) {
            d0->mem.release(d0->lockstep_imp_ptrs);
            d0->lockstep_imp_ptrs = nullptr;
            WGS_TRY(dev_alloc(d0, &d0->lockstep_imp_ptrs, num_slabs));
            d0->lockstep_imp_n = num_slabs;
        }
        HIP_TRY(hipMemcpyAsync(d0->lockstep_imp_ptrs, host.data(), sizeof(int32_t *) * num_slabs, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));  // (host vector goes out of scope)
        imp_ptrs = d0->lockstep_imp_ptrs;
    }
    for (uint32_t r = 0; r < num_slabs; r++) WGS_TRY(maintain_grid(slabs[r]));
    for (uint32_t i = 0; i < num_substeps; i++) {
        for (uint32_t r = 0; r < num_slabs; r++) WGS_TRY(shard_phase_begin(pipeline, slabs[r]));
        for (uint32_t r = 0; r + 1 < num_slabs; r++) {  // face between slab r and r + 1: the transport
            ShardLink &A = *slabs[r]->link, &B = *slabs[r + 1]->link;
            HIP_TRY(hipMemcpyAsync(B.msg_in[0], A.msg_out[1], A.msg_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(A.msg_in[1], B.msg_out[0], A.msg_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        for (uint32_t r = 0; r < num_slabs; r++) {
            slabs[r]->reduce_impulses = imp_ptrs ? 2 : 0;  // 2: bodies are integrated after the group-wide sum below
            WGS_TRY(shard_phase_end(pipeline, slabs[r]));
        }
        if (imp_ptrs) {
            hipLaunchKernelGGL(k_impulses_allreduce_local, dim3(1), dim3(128), 0, s, imp_ptrs, (int)num_slabs);
            for (uint32_t r = 0; r < num_slabs; r++) WGS_TRY(enqueue_bodies(slabs[r]));
        }
    }
    HIP_TRY(hipGetLastError());
    for (uint32_t r = 0; r < num_slabs; r++) WGS_TRY(watch_counters(slabs[r]));
    return loan.hand_back_waiting();
}

}  // extern "C"
