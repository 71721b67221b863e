// g2p_body.inc — the body of the fused G2P + particle-update kernels (see kernels_transfer.h), included textually so
// that the two-body launch of collider simulations (k_g2p_pair) compiles the very code of the single-body kernel.
// Expects in scope: d, side, epoch, the template parameters D / MODEL / PLASTIC / SHARD, the shared arrays s_node / s_cdf,
// and the macros G2P_CMODE, G2P_BX, G2P_GX (index of the workgroup within this body and their number).
// MODEL: 0 corotated, 1 neo-Hookean, 2 fluid — one model for every particle — or 3: every particle under its OWN model, a byte that
// travels with it (Dev::pmodel; loaded beside the pid through the sort permutation, stored beside it at the sorted slot). Only the
// particle update knows: the transfer, the binning and the CPIC paths are those of the other models, word for word.
// MODEL 4: the corotated model under the SNOW plasticity rule (WGS_PLASTICITY_SNOW, device_math.h snow_project; PLASTIC only). A value
// of MODEL rather than a parameter of its own: every instantiation that existed keeps its name and its code, and the plastic pair —
// beyond the instruction cache as it is — carries no branch for a rule it does not run. Everywhere but in the plastic block and at
// the stress it is MODEL 0 (`COROT`).
// SHARD: the data is one slab of a decomposition (particle counts in device counters, guests dropped, leavers listed).
// A template parameter rather than the run-time field it mirrors: this kernel lives at the limit of its scalar
// registers, and the single-domain instantiation should not carry a single one of them for a decomposition.
    constexpr bool CPIC = G2P_CMODE == 2;
    constexpr int BW = Dim<D>::BW, BS = Dim<D>::BSHIFT, TW = Dim<D>::TW, TILE = Dim<D>::TILE, NN = Dim<D>::NNBR;
    constexpr int DD = D * D;
    constexpr bool COROT = MODEL == 0 || MODEL == 4;
    static_assert(MODEL != 4 || PLASTIC, "the snow rule lives in the plastic block");
    // the node tile staged slice by slice (below): the one-chunk main body of the neo-Hookean elastic kernels in 3D on single-domain data — the
    // headline's pair and its collider-free twin, the two instantiations the change was timed on (notes/round_15.md). The list walk and the
    // multi-chunk kernels keep a staged tile across chunks, 2D tiles have no slices; the other models' one-chunk kernels, the plastic ones and a
    // slab's would take the same text and keep the whole tile until somebody times them.
    constexpr bool SLICES = D == 3 && G2P_CMODE != 2 && npass == 1u && MODEL == 1 && !PLASTIC && !SHARD;
    using P = Pl<D>;

    const float *in = d.buf[side];
    float *out = d.buf[side ^ 1];
    const uint32_t npad = d.npad;
    const float h = d.h, inv_h = d.inv_h;
    const float dt = d.sp->dt;
    const float invd = 4.0f / (h * h);  // kernel.wgsl:56-58
    const int tid = threadIdx.x;

    // XCD-aware mapping: workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its own L2. Every XCD
    // gets one contiguous eighth of the work — of the sorted particles (G2P_CMODE 0 / 1), of the visit list (2) —, so
    // that the ~8 waves that share a block (and therefore its node tile) hit the same L2 instead of eight different
    // ones. The eighths are eighths of the VALID particles: a sharded run launches for its capacity, and eighths of
    // that would leave the last XCDs without work.
    // A wave advances runs of `npass` consecutive items: chunks of 64 sorted particles (G2P_CMODE 0 / 1: one run per
    // wave), or entries of the visit list (2: the wave strides over the runs of its XCD's eighth; an entry = one chunk
    // that holds particles of one block near a collider, written by the sort, k_regroup). With more than one item per
    // run, the particle state of item p + 1 and the sort entries of item p + 2 are requested while item p is computed:
    // the wave pays the exposed sort-entry -> state latency (~3.4 of its ~7.5 us per chunk) once per run instead of
    // once per chunk, and a later item usually finds its block's node tile in LDS (kernels_transfer.h: which scenes
    // get how many).
    const uint32_t nvalid = SHARD ? ctr_cur(d, CTR_NV) : d.nv;   // sorted particles (num_valid, layout.h)
    const uint32_t per_xcd = (((nvalid + 64u * npass - 1u) / (64u * npass)) + 7u) >> 3;   // g2p_waves_per_xcd
    // The sorted order holds every particle unless the sort had to leave some out (grid overflow, key range:
    // reported). The entries behind the scan's total are then those of an earlier substep: advancing them would put a particle
    // into the output twice, and the block totals this launch keeps incrementally (Dev::bin_next) would no longer be counts.
    const uint32_t nsorted = min(nvalid, d.counters[CTR_NSORTED]);
    if constexpr (G2P_CMODE != 2) {
        if ((G2P_BX >> 3) >= per_xcd) return;
    }
    const uint32_t chunk0 = ((G2P_BX & 7u) * per_xcd + (G2P_BX >> 3)) * npass;
    uint32_t run = 0u, run_end = 0u, nvis = 0u;
    if constexpr (G2P_CMODE == 2) {
        nvis = min(d.counters[ctr_nvisit(G2P_BX & 7u, epoch)], d.visit_cap);  // the list of this XCD
        run = G2P_BX >> 3;
        run_end = (nvis + npass - 1u) / npass;
    }
    if constexpr (G2P_CMODE == 2) {
        // the colliders' motion -> LDS, once per wave (poses are integrated between the substeps, never inside this launch): the CPIC
        // stencil asks for a collider's velocity per incompatible (particle, node) pair, and every such question was two dependent
        // global loads and a full drain of the wave's memory counter in the middle of the stencil
        for (uint32_t i = (uint32_t)tid; i < min(d.n_colliders, 16u) * 9u; i += G2P_THREADS)
            reinterpret_cast<float *>(s_col)[i] = reinterpret_cast<const float *>(&d.colliders[i / 9u].linvel)[i % 9u];   // (linvel, angvel, com: nine consecutive floats)
        __syncthreads();
    }
    uint32_t chunk = chunk0, only = NONE;
    // does this body advance the particle of a sort entry? (G2P_CMODE 2: `blk` = the listed block the visit is about)
    auto g2p_wanted = [&](uint32_t entry, uint32_t blk) -> bool {
        if (entry == NONE) return false;
        // (not the main body's listed lanes: the test is two instructions in front of every pass's loads, and the headline — no listed
        // block at all — paid 1-2 us for them; at C3 it saved 130 MB of reads a launch, 1.5 % of the fused G2P)
        if constexpr (G2P_CMODE == 2) return ((entry & ~CELL_LISTED) >> 6) == blk;
        return true;
    };
    uint32_t staged = NONE;  // block whose node tile is in LDS
    uint32_t keyed = NONE, keyed_key = 0u;  // the block whose packed key is in a register, and that key
    uint32_t stamped = NONE; // Dev::bin_next: block whose "+" neighbours this wave activated last (consecutive items mostly share it)
    unsigned long long prof_visits = 0ull;
    G2P_PROF_LIST(0, wall_clock64())
    for (;;) {  // G2P_CMODE 2: the runs of this wave; 0 / 1: once
    // (block, chunk) of the items p .. p + 3 of the run (G2P_CMODE 2; wave-uniform). NONE: past the end of the list.
    uint2 e0 = make_uint2(NONE, NONE), e1 = e0, e2 = e0, e3 = e0;
    if constexpr (G2P_CMODE == 2) {
        if (run >= run_end) break;
        const uint32_t v0 = run * npass;
        const uint2 *vl = d.visit_list + (size_t)(G2P_BX & 7u) * d.visit_cap;
        e0 = vl[v0];
        if (npass > 1u && v0 + 1u < nvis) e1 = vl[v0 + 1u];
        if (npass > 2u && v0 + 2u < nvis) e2 = vl[v0 + 2u];
        if (npass > 3u && v0 + 3u < nvis) e3 = vl[v0 + 3u];
        static_assert(npass <= 4u, "the visit entries of a run are held in four registers");
    }
    // state of the next item (requested one pass ahead) and the sort entries of the item after it
    uint32_t nx_src = 0u, nx_cid = NONE, nx_pid = 0u, nn_src = 0u, nn_cid = NONE;
    [[maybe_unused]] uint32_t nx_pm = 0u;   // MODEL 3: the next item's model byte
    uint32_t nx_listed = 0u;  // G2P_CMODE 1: block_cpic of the next item's block (one more dependent load taken off the pass)
    float4 nx_xm = make_float4(0.f, 0.f, 0.f, 0.f), nx_f0 = nx_xm, nx_f1 = nx_xm, nx_f2 = nx_xm;
    if constexpr (npass > 1u) {
        const uint32_t c1 = G2P_CMODE == 2 ? e1.y : chunk0 + 1u;
        const uint32_t j1 = c1 * G2P_THREADS + tid;
        if (c1 != NONE && j1 < nsorted) {
            nx_src = d.perm[j1];
            nx_cid = d.perm_cell[j1];
        }
        if constexpr (npass > 2u) {
            const uint32_t c2 = G2P_CMODE == 2 ? e2.y : chunk0 + 2u;
            const uint32_t j2 = c2 * G2P_THREADS + tid;
            if (c2 != NONE && j2 < nsorted) {
                nn_src = d.perm[j2];
                nn_cid = d.perm_cell[j2];
            }
        }
    }
    for (int pass = 0; pass < (int)npass; pass++) {
        if constexpr (G2P_CMODE != 2) chunk = chunk0 + (uint32_t)pass;
        if constexpr (G2P_CMODE == 2) {
            if (pass >= 1) { e0 = e1; e1 = e2; e2 = e3; e3 = make_uint2(NONE, NONE); }
            only = e0.x;
            chunk = e0.y;
            if (chunk == NONE) break;  // the list ended inside this run
            prof_visits++;
        }
        const uint32_t chunk_p2 = G2P_CMODE == 2 ? e2.y : chunk + 2u;  // (where the item after the next one lives)

        G2P_PROF(0)
        const uint32_t j = chunk * G2P_THREADS + tid;  // slot in sorted order = output index
        const bool valid = j < nsorted;
        const bool second = npass > 1u && pass >= 1;  // this pass's state was requested one pass ago
        // (a first pass asks for its sort entries wherever the slot EXISTS — j < nvalid, a kernel argument on single-domain data —, not
        // where it is sorted — j < nsorted, a device counter: the request would wait for the counter's scalar load; what it fetched for a
        // slot behind the scan's total is dropped here)
        // (round 6, list walk) the "+" links of the visit's block — what the staging of its node-cdf tile waits for first — asked for with the sort entries:
        // a visit's chain was visit entry -> sort entries -> links -> node cdfs, four dependent round trips for 64 particles; now three
        uint32_t visit_link = NONE;
        if constexpr (G2P_CMODE == 2 && CPIC) {
            if (only != staged && tid < 8) visit_link = d.nbr_plus[only * 8u + (uint32_t)tid];
        }
        const bool inb = SHARD ? valid : j < nvalid;
        const uint32_t cid_ld = second ? nx_cid : (inb ? d.perm_cell[j] : NONE);
        const uint32_t cid_raw = valid ? cid_ld : NONE;
        // (the two sort entries of a slot are requested TOGETHER: asked for only where the first says the particle is this body's, the
        // second waited for the first — a dependent round trip in front of every wave's state loads, ~1.2 us of a wave's ~6.5 at the headline)
        // (not the neo-Hookean four-chunk kernel — C5's: only a quarter of its passes are first passes, and with the earlier request it
        // ran 613 -> 648 us, twice, on one box beside the dependent form; the corotated four-chunk kernel — C4's — gains 8-18 us)
        // (MODEL 3 sides with the corotated kernel here and at the block id below. Both choices follow the register allocation, and the
        // mixed kernel's is the corotated one's: its three stress branches are alternatives whose registers overlap, and the SVD
        // branch is by far the widest, so the kernel sits at MODEL 0's register count in every shape (notes/round_11.md: 166-168
        // VGPRs at the 168 cap in 3D, 8-20 B more scratch per lane than MODEL 0 where that one spills at all — the model byte and its
        // prefetched copy are two more values live across the pass). What upset the neo-Hookean kernels was measured on THEIR
        // allocation, which does not exist once the SVD is compiled in. Neither alternative was timed for MODEL 3.)
        constexpr bool together = npass <= 2u || COROT || MODEL == 3;
        const uint32_t src_any = second ? nx_src : (((together ? inb : valid) && (together || g2p_wanted(cid_raw, only))) ? d.perm[j] : 0u);
        // (a visit's lane whose particle belongs to another block than the listed one asks for slot 0 instead of its particle)
        const uint32_t src = (second || g2p_wanted(cid_raw, only)) ? src_any : 0u;
        const uint32_t cid = cid_raw == NONE ? NONE : (cid_raw & ~CELL_LISTED);  // physical block id * 64 + cell in block
        uint32_t myblock = cid == NONE ? NONE : (cid >> 6);
        if constexpr (G2P_CMODE == 1) {
            // lanes whose block belongs to the other launch drop out before touching particle state
            if (d.listed_in_perm) {  // (uniform) the sort entry says so
                if (cid_raw != NONE && (cid_raw & CELL_LISTED)) myblock = NONE;
            } else if (myblock != NONE && ((D == 3 && second) ? nx_listed : d.block_cpic[myblock]) != 0u) myblock = NONE;  // (2D: no prefetch of particle state)
        }
        if constexpr (G2P_CMODE == 2) {
            if (myblock != only) myblock = NONE;
        }

        // Particle state: issued before the tile staging so both latencies overlap.
        float x[D], Fm[DD], mass, vol0, lambda, mu;
        uint32_t pid;
        [[maybe_unused]] uint32_t pm = 0u;   // MODEL 3: this particle's model
        if constexpr (D == 3) {
            float4 xm, f0, f1, f2 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (second) {
                xm = nx_xm; f0 = nx_f0; f1 = nx_f1; f2 = nx_f2; pid = nx_pid;
                if constexpr (MODEL == 3) pm = nx_pm;
            } else {
                xm = ldq_stream(in, npad, P::XM, src);
                f0 = ldq_stream(in, npad, P::F0, src);
                f1 = ldq_stream(in, npad, P::F1, src);
                if (!d.uniform) f2 = ldq_stream(in, npad, P::F2, src);
                pid = ldpid<D>(in, npad, src);
                if constexpr (MODEL == 3) pm = ldmodel(d.pmodel[side], src);
            }
            if constexpr (npass > 1u) {
                if (pass + 1 < (int)npass) {  // the next pass's state, in flight while this one is computed
                    if constexpr (npass > 2u) {
                        if (pass >= 1) {  // its sort entries arrived a pass ago; request those of the pass after it
                            nx_src = nn_src;
                            nx_cid = nn_cid;
                            const uint32_t j2 = chunk_p2 * G2P_THREADS + tid;
                            nn_src = 0u;
                            nn_cid = NONE;
                            if (pass + 2 < (int)npass && chunk_p2 != NONE && j2 < nsorted) {
                                nn_src = d.perm[j2];
                                nn_cid = d.perm_cell[j2];
                            }
                        }
                    }
                    if (!g2p_wanted(nx_cid, e1.x)) nx_src = 0u;   // (not this body's: slot 0 — above)
                    nx_xm = ldq_stream(in, npad, P::XM, nx_src);
                    nx_f0 = ldq_stream(in, npad, P::F0, nx_src);
                    nx_f1 = ldq_stream(in, npad, P::F1, nx_src);
                    if (!d.uniform) nx_f2 = ldq_stream(in, npad, P::F2, nx_src);
                    nx_pid = ldpid<D>(in, npad, nx_src);
                    if constexpr (MODEL == 3) nx_pm = ldmodel(d.pmodel[side], nx_src);
                    if constexpr (G2P_CMODE == 1) {
                        if (!d.listed_in_perm) nx_listed = nx_cid != NONE ? d.block_cpic[(nx_cid & ~CELL_LISTED) >> 6] : 0u;
                    }
                }
            }
            x[0] = xm.x; x[1] = xm.y; x[2] = xm.z;
            Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
            Fm[4] = f1.x; Fm[5] = f1.y; Fm[6] = f1.z; Fm[7] = f1.w;
            if (d.uniform) {  // one material: the constants are kernel arguments, F[8] rides in XM.w (layout.h)
                Fm[8] = xm.w; mass = d.uni_mass; vol0 = d.uni_vol; lambda = d.uni_lambda; mu = d.uni_mu;
            } else {
                mass = xm.w;
                Fm[8] = f2.x; vol0 = f2.y; lambda = f2.z; mu = f2.w;
            }
        } else {
            const float4 xm = ldq_stream(in, npad, P::XM, src);
            const float4 f0 = ldq_stream(in, npad, P::F0, src);
            const float4 vl = ldq_stream(in, npad, P::CV2, src);
            x[0] = xm.x; x[1] = xm.y; mass = xm.z; vol0 = xm.w;
            Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
            lambda = vl.z; mu = vl.w;
        }
        if constexpr (D == 2) pid = ldpid<D>(in, npad, src);
        if constexpr (D == 2 && MODEL == 3) pm = ldmodel(d.pmodel[side], src);

        float pvel[D], nrm[D], sdist = 0.f;
        uint32_t paff = 0;
        if constexpr (CPIC) {
            const float4 c0 = ldq_stream(in, npad, P::CDF0, src);
            nrm[0] = c0.x; nrm[1] = c0.y;
            if constexpr (D == 3) {
                const float4 cv = ldq_stream(in, npad, P::CV2, src);
                const float4 c1 = ldq_stream(in, npad, P::CDF1, src);
                nrm[2] = c0.z; sdist = c0.w; paff = __float_as_uint(c1.w);
                pvel[0] = cv.y; pvel[1] = cv.z; pvel[2] = cv.w;
            } else {
                const float4 vl = ldq_stream(in, npad, P::CV2, src);
                sdist = c0.z; paff = __float_as_uint(c0.w);
                pvel[0] = vl.x; pvel[1] = vl.y;
            }
        }

#ifdef WGS_ABLATE
        if (d.dbg & DBG_ABLATE_G2P_BYTES_ONLY) {  // ablation: memory traffic of the kernel without tile staging / maths
            if (valid) {
                if constexpr (D == 3) {
                    stq(out, npad, P::XM, j, make_float4(x[0], x[1], x[2], mass));
                    stq(out, npad, P::CV0, j, make_float4(Fm[0], Fm[1], Fm[2], Fm[3]));
                    stq(out, npad, P::CV1, j, make_float4(Fm[4], Fm[5], Fm[6], Fm[7]));
                    stq(out, npad, P::CV2, j, make_float4(Fm[8], x[0], x[1], x[2]));
                    stq(out, npad, P::F0, j, make_float4(Fm[0], Fm[1], Fm[2], Fm[3]));
                    stq(out, npad, P::F1, j, make_float4(Fm[4], Fm[5], Fm[6], Fm[7]));
                    stq(out, npad, P::F2, j, make_float4(Fm[8], vol0, lambda, mu));
                }
                stpid<D>(out, npad, j, pid);
                if constexpr (MODEL == 3) stmodel(d.pmodel[side ^ 1], j, pm);
            }
            G2P_DONE;
        }
#endif
        G2P_PROF(1)
        unsigned long long todo = __ballot(myblock != NONE);
        while (todo) {  // wave-uniform: one iteration per distinct block among the 64 particles (1 or 2)
            const int leader = __ffsll((long long)todo) - 1;
            // (the block of the leader: by v_readlane — the id then lives in a scalar register and the kernels shed 4-32 B of scratch per
            // lane: C4's fused G2P 445 -> 413 us — except in the neo-Hookean elastic kernels, whose allocation the same change upsets:
            // the headline's ran 44.8 -> 46.5 us over five alternations on one box, C5's was a wash. They keep the permute.)
            const uint32_t b = (COROT || MODEL == 3 || PLASTIC) ? lane_value(myblock, leader) : (uint32_t)__shfl(myblock, leader);
            const bool mine = myblock == b;
            todo &= ~__ballot(mine);
            int bc[3] = {0, 0, 0};
            // (the key of the block handled last stays in a register: a load here stands in front of everything the item does, and
            // behind the acknowledgements of the previous item's stores — loads and stores share one counter, in order)
            const uint32_t bkey = b == keyed ? keyed_key : d.block_key[b];
            keyed = b;
            keyed_key = bkey;
            unpack_key<D>(bkey, bc);
            // Dev::bin_next: this launch also BINS its output for the next substep — what launch 1 of the next
            // sort (k_rebin, kernels_sort.h: sort.wgsl:26-36,89-99 for a buffer in sorted order) would do from the stored
            // positions is done here from the registers that hold them: the new cell id of every particle, the activation of its
            // block and that block's "+" neighbours (idempotent stamp stores through this substep's links) and, for the particles
            // that changed cell, the push on the destination cell's list. The per-block totals are not recounted: block_acc
            // persists from substep to substep and only a particle that changes BLOCK moves one unit from its old block to its
            // new one (the grid update leaves block_acc alone in such a substep). A launch, its 16 MB re-read of the positions
            // and an atomic per wave go. Everything that RETURNS a value (the list push, the destination block's links) is
            // requested before the constitutive update: a load issued behind the output stores waits for their acknowledgement
            // (one vmcnt for both: requested at the very end, the wave's own links alone doubled this launch's time). The ids of
            // b's neighbours are staged in LDS with the node tile.
            bool stays = false;   // this lane's particle is still in block b after the update
            bool moved = false;   // ... it changed cell (or was dropped)
            if (SHARD && d.skip_guests && (bc[0] < d.shard_lo || bc[0] >= d.shard_hi)) {  // (wave-uniform) a block of GUESTS: particles that
                // left the core range one substep ago. This rank transferred them to the grid once more; their record
                // travelled with this substep's node sums and the new owner advances them (kernels_shard.h k_g2p_arrivals).
                if (mine) stpid<D>(out, npad, j, PID_DEAD);
                if constexpr (G2P_BIN) {   // (Dev::bin_next, below) they are out of this rank's next sort: nobody's cell, b's total less, b's run changed
                    if (d.bin_next) {
                        const uint32_t gone = (uint32_t)__popcll(__ballot(mine));
                        if (mine) d.cellid[j] = NONE;
                        if (tid == leader) {
                            atomicAdd(&d.block_acc[b], 0u - gone);
                            d.block_dirty[b] = epoch + 1u;
                        }
                    }
                }
                continue;
            }
            if (b != staged) {  // (the next item of a run usually continues in the same block)
                __syncthreads();  // single-wave workgroup: orders the LDS tile reuse
                // g2p.wgsl:72-132: velocities of the block's nodes and of its +1 rim -> LDS tile. The grid
                // update left them in the block's own slab, so this is one contiguous read.
                // (the slab is stored by regions, layout.h: read linearly, placed by tile index)
                // (the tile index of a slab position comes from a table in constant memory, fetched with the slab itself;
                // the slice-wise staging walks in tile order and computes the slab position: layout.h slab_pos_of_tile)
                if constexpr (SLICES) {
                    // One chunk per wave, in 3D: only the z-slices of the tile that this chunk's cells of b reach. A chunk covers consecutive
                    // cells of the sorted order — at 8 particles per cell half a z-layer of the block —, and a particle in cell layer z reads
                    // the slices z .. z + 2: 108 of the 216 nodes, two rounds of slab loads and LDS writes per lane instead of four. The
                    // layers come from the lanes this body advances in b (four ballots, scalar); LDS is indexed by tile node as before.
                    const uint32_t lz = (cid >> (2 * BS)) & (uint32_t)(BW - 1);
                    uint32_t zmask = 0u;
    #pragma unroll
                    for (int k = 0; k < BW; k++) zmask |= __ballot(mine && lz == (uint32_t)k) != 0ull ? 1u << k : 0u;
                    const int n0 = (__ffs((int)zmask) - 1) * TW * TW, n1 = (32 - __clz((int)zmask) + 2) * TW * TW;
                    // (every load before the first LDS write, like the unrolled whole-tile loop; a lane past the end asks for the last node
                    // again instead of leaving the round through a branch; the rounds nobody needs are skipped by the whole wave)
                    static_assert(!SLICES || (TILE > 3 * G2P_THREADS && TILE <= 4 * G2P_THREADS && 3 * TW * TW > G2P_THREADS), "four rounds at most, the first two always");
                    auto slab_node = [&](int r) -> float4 {
                        const uint32_t sp = slab_pos_of_tile<D>((uint32_t)min(n0 + r * G2P_THREADS + tid, n1 - 1));
                        return d.slab[(size_t)b * TILE + sp];
                    };
                    const bool r2 = n0 + 2 * G2P_THREADS < n1, r3 = n0 + 3 * G2P_THREADS < n1;   // (wave-uniform)
                    const float4 q0 = slab_node(0), q1 = slab_node(1);
                    float4 q2 = make_float4(0.f, 0.f, 0.f, 0.f), q3 = q2;   // (not copies of q1: a copy waits for q1)
                    if (r2) q2 = slab_node(2);
                    if (r3) q3 = slab_node(3);
                    s_node[n0 + tid] = q0;
                    if (n0 + G2P_THREADS + tid < n1) s_node[n0 + G2P_THREADS + tid] = q1;
                    if (n0 + 2 * G2P_THREADS + tid < n1) s_node[n0 + 2 * G2P_THREADS + tid] = q2;
                    if (n0 + 3 * G2P_THREADS + tid < n1) s_node[n0 + 3 * G2P_THREADS + tid] = q3;
                    // (`staged = b` below then names a PARTLY staged tile. Nobody can take it for a whole one: with one chunk per wave the
                    // outer loop runs once and `while (todo)` meets every block once. A kernel that revisits a block must not set SLICES.)
                } else {   // the whole tile, for the chunks and visits that follow in this wave
                    for (int n = tid; n < TILE; n += G2P_THREADS) {
                        uint32_t np = (uint32_t)n;
                        // (pinned in the list walk: slab + 16 n would otherwise live as a 64-bit loop invariant per round — in scratch, there)
                        if constexpr (G2P_CMODE == 2) asm volatile("" : "+v"(np));
                        s_node[g_slab_tile_map.t[n]] = d.slab[(size_t)b * TILE + np];
                    }
                }
                if constexpr (CPIC) {
                    if constexpr (G2P_CMODE == 2) stage_node_cdf_tile_links<D, G2P_THREADS>(d, visit_link, s_cdf, tid);   // (b is the visit's block: its links are here)
                    else stage_node_cdf_tile<D, G2P_THREADS>(d, b, s_cdf, tid);
                }
                if constexpr (G2P_BIN) {   // ids of b's "+" and "-" neighbours, if they are in the table: where a particle that leaves b goes
                    if (d.bin_next && tid < 16) s_nbr[tid] = d.nbr_known[b * 16u + (uint32_t)tid];
                }
                __syncthreads();
                staged = b;
            }

            G2P_PROF(2)
            if (mine) {
                // ---- G2P (g2p.wgsl:150-218)
                // The associated cell comes from the sort (perm_cell = block * 64 + cell in block, computed
                // by k_bin from this very position with the bit-exact rule), so no fp32 division here.
                float ref[D], w[D][3];
                int tbase = 0;
                {
                    const uint32_t lc = cid & 63u;
                    int lcell[3] = {(int)(lc & (BW - 1)), (int)((lc >> BS) & (BW - 1)), D == 3 ? (int)(lc >> (2 * BS)) : 0};
                    int stride = 1;
    #pragma unroll
                    for (int k = 0; k < D; k++) {
                        ref[k] = (float)(bc[k] * BW + lcell[k]) * h - x[k];
                        eval_all(-ref[k] * inv_h, w[k]);
                        tbase += lcell[k] * stride;
                        stride *= TW;
                    }
                }
                float vel[D], grad[DD];
                constexpr int SZN = D == 3 ? 3 : 1;
                // CPIC body: a particle all of whose stencil nodes are compatible with it (g2p.wgsl:183-199 then takes the
                // node's own velocity everywhere) — most particles of a block near a collider, everything but the layer
                // against it — is transferred like a particle of the plain body, by the tensor-product evaluation; the
                // 27-term form with its per-node tests is left to the others. Decided per particle (a lane takes the
                // path its own 27 tests select, whoever shares its wave), skipped per wave when no lane needs a path.
                bool plain_lane = !CPIC;
                if constexpr (CPIC) {
                    uint32_t incompatible = 0u;
    #pragma unroll 1
                    for (int sz = 0; sz < SZN; sz++)
    #pragma unroll
                        for (int sy = 0; sy < 3; sy++)
    #pragma unroll
                            for (int sx = 0; sx < 3; sx++)
                                incompatible |= affinities_are_compatible(paff, s_cdf[tbase + sx + TW * sy + (D == 3 ? TW * TW * sz : 0)].affinities) ? 0u : 1u;
                    plain_lane = incompatible == 0u;
                }
                if (plain_lane) {
                    // Tensor-product evaluation of
                    //   v = sum_n w_n v_n ,  G_c = sum_n w_n s_c(n) v_n   (s = node offset in {0,1,2}^D)
                    // reducing along x, then y, then z: ~240 VALU instead of ~570 for the 27 direct terms.
                    // grad = inv_d * sum_n w_n v_n (x) (ref + s h) = inv_d * (v (x) ref + h * [G_x G_y G_z]).
                    float G[D][D];  // G[c][r]
    #pragma unroll
                    for (int k = 0; k < D; k++) vel[k] = 0.f;
    #pragma unroll
                    for (int c = 0; c < D; c++)
    #pragma unroll
                        for (int r = 0; r < D; r++) G[c][r] = 0.f;
                    const float wx1 = w[0][1], wx2 = 2.0f * w[0][2];
    #pragma unroll 1
                    for (int sz = 0; sz < SZN; sz++) {
                        float Pz[D], Gxz[D], Gyz[D];
    #pragma unroll
                        for (int k = 0; k < D; k++) { Pz[k] = 0.f; Gxz[k] = 0.f; Gyz[k] = 0.f; }
    #pragma unroll
                        for (int sy = 0; sy < 3; sy++) {
                            const int idx = tbase + TW * sy + (D == 3 ? TW * TW * sz : 0);
                            const float4 n0 = s_node[idx], n1 = s_node[idx + 1], n2 = s_node[idx + 2];
                            float a0[3] = {n0.x, n0.y, n0.z}, a1[3] = {n1.x, n1.y, n1.z}, a2[3] = {n2.x, n2.y, n2.z};
                            const float wy = w[1][sy];
    #pragma unroll
                            for (int k = 0; k < D; k++) {
                                const float p = w[0][0] * a0[k] + w[0][1] * a1[k] + w[0][2] * a2[k];
                                const float gx = wx1 * a1[k] + wx2 * a2[k];
                                Pz[k] += wy * p;
                                Gxz[k] += wy * gx;
                                if (sy > 0) Gyz[k] += ((float)sy * wy) * p;
                            }
                        }
                        float wz = 1.f;
                        if constexpr (D == 3) wz = sz == 0 ? w[2][0] : (sz == 1 ? w[2][1] : w[2][2]);
    #pragma unroll
                        for (int k = 0; k < D; k++) {
                            vel[k] += wz * Pz[k];
                            G[0][k] += wz * Gxz[k];
                            G[1][k] += wz * Gyz[k];
                            if constexpr (D == 3) G[2][k] += ((float)sz * wz) * Pz[k];
                        }
                    }
    #pragma unroll
                    for (int c = 0; c < D; c++)
    #pragma unroll
                        for (int r = 0; r < D; r++) grad[c * D + r] = invd * (vel[r] * ref[c] + h * G[c][r]);
                }
                if (CPIC && !plain_lane) {
    #pragma unroll
                    for (int k = 0; k < D; k++) vel[k] = 0.f;
    #pragma unroll
                    for (int k = 0; k < DD; k++) grad[k] = 0.f;
                    // The z loop is kept rolled on purpose: fully unrolled, hipcc issues all 27
                    // ds_read_b128 up front (108 VGPRs of tile values) and the kernel drops to 2 waves/SIMD.
    #pragma unroll 1
                    for (int sz = 0; sz < SZN; sz++)
    #pragma unroll 1
                        for (int sy = 0; sy < 3; sy++)
    #pragma unroll 1
                            for (int sx = 0; sx < 3; sx++) {
                                const int idx = tbase + sx + TW * sy + (D == 3 ? TW * TW * sz : 0);
                                float4 nd = s_node[idx];
                                float nv[D];
                                nv[0] = nd.x; nv[1] = nd.y;
                                if constexpr (D == 3) nv[2] = nd.z;
                                float dpt[D];
                                dpt[0] = ref[0] + (float)sx * h;
                                dpt[1] = ref[1] + (float)sy * h;
                                if constexpr (D == 3) dpt[2] = ref[2] + (float)sz * h;
                                float wgt = w[0][sx] * w[1][sy];
                                if constexpr (D == 3) wgt *= (sz == 0 ? w[2][0] : (sz == 1 ? w[2][1] : w[2][2]));
                                NodeCdf nc = s_cdf[idx];
                                if (!affinities_are_compatible(paff, nc.affinities)) {
                                    if (nc.closest_id != NONE && nc.closest_id < d.n_colliders) {
                                        const ColliderMotion &col = s_col[nc.closest_id];
                                        float cc[D], bv[D], rel[D], pr[D];
    #pragma unroll
                                        for (int k = 0; k < D; k++) cc[k] = dpt[k] + x[k];
                                        velocity_at_point<D>(col, cc, bv);
    #pragma unroll
                                        for (int k = 0; k < D; k++) rel[k] = pvel[k] - bv[k];
                                        project_velocity<D>(rel, nrm, pr);
    #pragma unroll
                                        for (int k = 0; k < D; k++) nv[k] = bv[k] + pr[k];
                                    } else {
    #pragma unroll
                                        for (int k = 0; k < D; k++) nv[k] = pvel[k];
                                    }
                                }
                                const float wi = wgt * invd;
    #pragma unroll
                                for (int k = 0; k < D; k++) vel[k] += nv[k] * wgt;
    #pragma unroll
                                for (int c = 0; c < D; c++)
    #pragma unroll
                                    for (int r = 0; r < D; r++) grad[c * D + r] += wi * (nv[r] * dpt[c]);
                            }
                }

                float rvel[D];
    #pragma unroll
                for (int k = 0; k < D; k++) rvel[k] = 0.f;
                if constexpr (CPIC) {  // g2p.wgsl:220-226 (bounded by the real collider count, quirk B9)
                    for (uint32_t c = 0; c < d.n_colliders && c < 16u; c++)
                        if (paff & (1u << c)) {
                            float bv[D];
                            velocity_at_point<D>(s_col[c], x, bv);
    #pragma unroll
                            for (int k = 0; k < D; k++) rvel[k] += bv[k];
                        }
                }

                G2P_PROF(3)
                // ---- particle update (particle_update.wgsl:58-132)
                if constexpr (CPIC) {
                    if (sdist < -0.05f * h) {
                        float rel[D], pr[D];
    #pragma unroll
                        for (int k = 0; k < D; k++) rel[k] = vel[k] - rvel[k];
                        project_velocity<D>(rel, nrm, pr);
    #pragma unroll
                        for (int k = 0; k < D; k++) vel[k] = rvel[k] + pr[k];
                    }
                }
                float l2 = 0.f;
    #pragma unroll
                for (int k = 0; k < D; k++) l2 += vel[k] * vel[k];
                const float len = sqrtf(l2);
                if (len > h / dt) {
    #pragma unroll
                    for (int k = 0; k < D; k++) vel[k] = vel[k] / len * h / dt;
                }
                float xn[D];
    #pragma unroll
                for (int k = 0; k < D; k++) xn[k] = x[k] + vel[k] * dt;
                if constexpr (SHARD) {  // a particle whose associated block left the core range is listed: next substep's guest (k_pack_face)
                    const int nbx = assoc_cell(xn[0], d.h, d.inv_h, d.h_pow2 != 0u) >> BS;
                    if (nbx < d.shard_lo || nbx >= d.shard_hi) {
                        const uint32_t ls = atomicAdd(&d.counters[CTR_NLEAVE], 1u);  // a handful per substep
                        if (ls < d.leavers_cap) d.leavers[ls] = j;
                        else atomicOr(&d.counters[CTR_ERRORS], ERRBIT_SHARD);
                    }
                }
                uint32_t mv_prev = 0u, cell_entry = NONE;
                bool is_mover = false;
                if constexpr (G2P_BIN) {
                    if (d.bin_next) {
                        const bool p2 = d.h_pow2 != 0u;
                        int nbk[3] = {0, 0, 0};
                        uint32_t bin_local = 0u, shift = 0u, dpos = 0u, dneg = 0u, dfar = 0u;
    #pragma unroll
                        for (int k = 0; k < D; k++) {
                            const int c = assoc_cell(xn[k], h, inv_h, p2);   // the bit-exact rule on the very value stored below
                            nbk[k] = c >> BS;
                            bin_local |= (uint32_t)(c & (BW - 1)) << shift;
                            shift += BS;
                            const int dk = nbk[k] - bc[k];
                            dpos |= dk == 1 ? (1u << k) : 0u;
                            dneg |= dk == -1 ? (1u << k) : 0u;
                            dfar |= (dk > 1 || dk < -1) ? 1u : 0u;
                        }
                        uint32_t ncid = NONE;
                        if ((dpos | dneg | dfar) == 0u) {   // still in its block, like nearly every particle (b and its "+" neighbours are representable: it was active)
                            stays = true;
                            ncid = b * NPB + bin_local;
                        } else {
                            // Few particles change block. The destination is a neighbour of b; when it lies on the "+" or on the "-"
                            // side in every axis it moved along (every face neighbour does) its id is in LDS.
                            int hi[3] = {nbk[0] + 1, nbk[1] + 1, nbk[2] + 1};
                            if (!block_in_key_range<D>(nbk) || !block_in_key_range<D>(hi)) {
                                atomicOr(&d.counters[CTR_ERRORS], ERRBIT_KEYRANGE);
                            } else {
                                const uint32_t nkey = pack_key<D>(nbk);
                                uint32_t y = NONE;
                                if (dfar == 0u && dneg == 0u) y = s_nbr[dpos];
                                else if (dfar == 0u && dpos == 0u) y = s_nbr[8u + dneg];
                                // (a "-" neighbour may be in the table without being active — and launch 2 of this substep's sort may have
                                // evicted it after noting its id: the key says. kernels_sort.h regroup_block)
                                if (y != NONE && d.block_key[y] != nkey) y = NONE;
                                // ONE copy of the insertion code (it is inlined, and this kernel answers to every instruction compiled into it):
                                // first the destination itself when it is not in the table — a diagonal neighbour, or a block nobody
                                // activated yet (bit 31 of `act`) —, then those of its "+" neighbours that its links of this substep do not
                                // reach (bits 0 .. 2^D - 1: the rim of the active region; all of them for a block inserted just now).
                                uint32_t act = y == NONE ? 0x80000000u : 0u;
                                bool linked = false;   // the destination's links have been looked at
    #pragma unroll 1
                                for (;;) {
                                    if (act == 0u && !linked) {
                                        linked = true;
                                        if (y != NONE) {
                                            const uint32_t le = d.links_epoch[y];
                                            uint32_t lk[NN];
    #pragma unroll
                                            for (int o = 0; o < NN; o++) lk[o] = d.nbr_plus[y * 8u + (uint32_t)o];
                                            ncid = y * NPB + bin_local;
                                            atomicAdd(&d.block_acc[y], 1u);   // sort.wgsl:89-99, incrementally: one particle more there
                                            // grid.wgsl:300-320: the destination and its "+" neighbours are active in the next substep — through its
                                            // links of this substep where it has them (the first is the block itself), through the hash map otherwise
    #pragma unroll
                                            for (int o = 0; o < NN; o++) {
                                                if (le == epoch && lk[o] != NONE) d.block_stamp[lk[o]] = epoch + 1u;
                                                else act |= 1u << o;
                                            }
                                        }
                                    }
                                    if (act == 0u) break;
                                    const bool dest = (act & 0x80000000u) != 0u;
                                    const int o = dest ? 0 : __ffs((int)act) - 1;
                                    int nb[3] = {nbk[0] + (o & 1), nbk[1] + ((o >> 1) & 1), nbk[2] + ((o >> 2) & 1)};
                                    uint32_t got = NONE;
                                    if (dest || block_in_key_range<D>(nb)) got = activate_block(d, dest ? nkey : pack_key<D>(nb), epoch + 1u);
                                    if (dest) {
                                        y = got < d.cap ? got : NONE;   // (NONE: grid overflow, reported — left out of the next substep)
                                        act = 0u;
                                    } else {
                                        act &= act - 1u;
                                    }
                                }
                            }
                            {   // ... and one less here (also when it left the key range or the grid overflowed)
                                // (runs of one or two chunks: the index pinned at the access — hipcc otherwise forms block_acc + 4 b at the top
                                // of the pass, a 64-bit pair that finds no register and is STORED TO SCRATCH by every wave for a path one
                                // particle in thirty takes: 8 of the 16 bytes per lane and pass that the headline wrote for nothing. The
                                // four-chunk kernels keep the hoisted form: pinned, C5's ran 4 % longer — its allocation follows no plan one can steer)
                                uint32_t bb = b;
                                if constexpr (npass <= 2u) asm volatile("" : "+v"(bb));
                                atomicAdd(&d.block_acc[bb], 0xffffffffu);
                            }
                        }
                        // (the entry itself is stored with the particle at the end: a store here would stand in front of every later load —
                        // one counter for both, in order — and the Drucker-Prager quads are requested right below: C3 + 100 us)
                        cell_entry = (ncid != NONE && ncid != cid) ? (ncid | CELL_MOVED) : ncid;
                        moved = ncid != cid;
                        // sort.wgsl:129-137, only for a particle that CAME FROM ANOTHER BLOCK: it is pushed on its new cell's list. One
                        // that changed cell inside its block is found by the wave that regroups the block (kernels_sort.h).
                        if (!stays && ncid != NONE) {   // (kernels_sort.h push_arrival, the position requested here and used at the end)
                            is_mover = true;
                            mv_prev = atomicAdd(&d.blk_narr[ncid >> 6], 1u);
                        }
                    }
                }
                if constexpr (CPIC) {
                    if (sdist < -0.05f * h) {
                        const float corrected = fmaxf(sdist, -0.3f * h);
                        const float imp = dt * -corrected * 1.0e3f;
    #pragma unroll
                        for (int k = 0; k < D; k++) vel[k] += imp * nrm[k];
                    }
                }
                // F <- F + (grad * dt) * F   (the fluid keeps J alone, in F[0]: fluid_update below)
                // (MODEL 3: where the particle is not fluid. A per-lane branch, like the stress below: a wave that holds one kind skips the
                // others' code, a mixed wave runs the branches it needs one after the other — the sum of the models it holds, never more)
                if (MODEL != 2 && (MODEL != 3 || pm != 2u)) {
                    float gdt[DD], prod[DD];
    #pragma unroll
                    for (int k = 0; k < DD; k++) gdt[k] = grad[k] * dt;
                    mat_mul<D>(gdt, Fm, prod);
    #pragma unroll
                    for (int k = 0; k < DD; k++) Fm[k] += prod[k];
                }

                float tau[DD];
                Svd<D> sv;
                if constexpr (PLASTIC) {
                    float dp[6], st[3], phase, max_stretch;
                    {
                        const float4 d1 = ldq_stream(in, npad, P::DP1, src);
                        if (d.uni_dp == 2u) {   // (uniform: all six parameters and max_stretch are kernel arguments, the state is ONE quad: layout.h)
#pragma unroll
                            for (int k = 0; k < 6; k++) dp[k] = d.uni_dpv[k];
                            st[0] = d1.x; st[1] = d1.y; st[2] = d1.z; phase = d1.w; max_stretch = d.uni_max_stretch;
                        } else {
                            const float4 d2 = ldq_stream(in, npad, P::DP2, src);
                            if (d.uni_dp == 1u) {   // (one set of h0..h3 for all particles)
                                dp[0] = d.uni_dpv[0]; dp[1] = d.uni_dpv[1]; dp[2] = d.uni_dpv[2]; dp[3] = d.uni_dpv[3];
                            } else {
                                const float4 d0 = ldq_stream(in, npad, P::DP0, src);
                                dp[0] = d0.x; dp[1] = d0.y; dp[2] = d0.z; dp[3] = d0.w;
                            }
                            dp[4] = d1.x; dp[5] = d1.y;
                            st[0] = d1.z; st[1] = d1.w; st[2] = d2.x; phase = d2.y; max_stretch = d2.z;
                        }
                    }
                    G2P_PROF(6)
                    // One SVD per particle, at one place in the code (the three consumers below share it; the kernel
                    // is already at the edge of the instruction cache): particle_update.wgsl:103,109 take it of the
                    // updated F, drucker_prager.wgsl:139 and linear_elasticity.wgsl:29 of the same matrix.
                    const bool breakable = phase > 0.f && max_stretch > 0.f;
                    if (MODEL != 1 || breakable || (phase == 0.f && dp[4] != 0.f)) svd<D>(Fm, sv);
                    G2P_PROF(7)
                    if (breakable) {  // particle_update.wgsl:98-116
                        bool broken = false;
    #pragma unroll
                        for (int k = 0; k < D; k++) broken = broken || sv.s[k] > max_stretch;
                        if (broken) phase = 0.f;
                    }
                    // (MODEL 4: the hardening factor of a snow particle — 1: the particle is not one — waits for the stress in tau[0], which nobody
                    // has written yet. Not a variable of its own: the instantiations of the other models would declare it too, and two of
                    // them came out of the compiler with a pair of instructions swapped)
                    if constexpr (MODEL == 4) tau[0] = 1.0f;
                    if (phase == 0.f && dp[4] != 0.f) {  // particle_update.wgsl:118-122, drucker_prager.wgsl:134
                        if constexpr (MODEL == 4) tau[0] = snow_project<D>(dp, st, Fm, sv);   // (the same gate, the other rule)
                        else drucker_prager_project<D>(dp, st, Fm, sv);  // sv.s follows the projected F
                    }
                    if (d.uni_dp == 2u) {
                        stq(out, npad, P::DP1, j, make_float4(st[0], st[1], st[2], phase));
                    } else {
                        if (d.uni_dp == 0u) stq(out, npad, P::DP0, j, make_float4(dp[0], dp[1], dp[2], dp[3]));   // (else: the quad is in both buffers already)
                        stq(out, npad, P::DP1, j, make_float4(dp[4], dp[5], st[0], st[1]));
                        stq(out, npad, P::DP2, j, make_float4(st[2], phase, max_stretch, 0.f));
                    }
                }
                if constexpr (MODEL == 3) {
                    static_assert(MODEL != 3 || !PLASTIC, "per-particle models: no plastic state (wgs_set_particle_models refuses such data)");
                    // the very functions of the three homogeneous instantiations, each on the arguments it gets there: under
                    // -ffp-contract=on the rounding of a branch is that of its own kernel
                    if (pm == 2u) {
                        Fm[0] = fluid_update<D>(lambda, mu, d.fluid_gamma, grad, dt, Fm[0], tau);
                    } else if (pm == 1u) {
                        kirchoff_neo_hookean<D>(lambda, mu, Fm, tau);
                    } else {
                        svd<D>(Fm, sv);
                        kirchoff_corotated<D>(lambda, mu, Fm, sv, tau);
                    }
                } else if constexpr (MODEL == 2) {
                    static_assert(MODEL != 2 || !PLASTIC, "the fluid carries no plastic state");
                    Fm[0] = fluid_update<D>(lambda, mu, d.fluid_gamma, grad, dt, Fm[0], tau);   // def_grad = diag(J, 1[, 1]): layout.h
                } else if constexpr (MODEL == 1) {
                    kirchoff_neo_hookean<D>(lambda, mu, Fm, tau);
                } else if constexpr (MODEL == 4) {
                    // lambda hf, mu hf with hf of the UPDATED Jp; the stored coefficients stay the particle's own (hf is never stored)
                    const float hf = tau[0];
                    kirchoff_corotated<D>(lambda * hf, mu * hf, Fm, sv, tau);
                } else {
                    if constexpr (!PLASTIC) svd<D>(Fm, sv);
                    kirchoff_corotated<D>(lambda, mu, Fm, sv, tau);
                }
                G2P_PROF(4)
                // particle_update.wgsl:129-132: C' = grad * m - tau * (V0 * inv_d * dt)
                const float coeff = vol0 * invd * dt;
                float Cn[DD];
    #pragma unroll
                for (int k = 0; k < DD; k++) Cn[k] = grad[k] * mass - tau[k] * coeff;
                if constexpr (D == 3) {
                    stq(out, npad, P::XM, j, make_float4(xn[0], xn[1], xn[2], d.uniform ? Fm[8] : mass));
                    stq(out, npad, P::CV0, j, make_float4(Cn[0], Cn[1], Cn[2], Cn[3]));
                    stq(out, npad, P::CV1, j, make_float4(Cn[4], Cn[5], Cn[6], Cn[7]));
                    stq(out, npad, P::CV2, j, make_float4(Cn[8], vel[0], vel[1], vel[2]));
                    stq(out, npad, P::F0, j, make_float4(Fm[0], Fm[1], Fm[2], Fm[3]));
                    stq(out, npad, P::F1, j, make_float4(Fm[4], Fm[5], Fm[6], Fm[7]));
                    if (!d.uniform) stq(out, npad, P::F2, j, make_float4(Fm[8], vol0, lambda, mu));
                } else {
                    stq(out, npad, P::XM, j, make_float4(xn[0], xn[1], mass, vol0));
                    stq(out, npad, P::CV0, j, make_float4(Cn[0], Cn[1], Cn[2], Cn[3]));
                    stq(out, npad, P::CV2, j, make_float4(vel[0], vel[1], lambda, mu));
                    stq(out, npad, P::F0, j, make_float4(Fm[0], Fm[1], Fm[2], Fm[3]));
                }
                stpid<D>(out, npad, j, pid);
                if constexpr (MODEL == 3) stmodel(d.pmodel[side ^ 1], j, pm);
                // G2P_CMODE 1 (no collider in reach): default_cdf() is implied by a stale stamp, nothing to store (layout.h)
                if constexpr (CPIC) {
                    if constexpr (D == 3) {
                        stq(out, npad, P::CDF0, j, make_float4(nrm[0], nrm[1], nrm[2], sdist));
                        stq(out, npad, P::CDF1, j, make_float4(rvel[0], rvel[1], rvel[2], __uint_as_float(paff)));
                    } else {
                        stq(out, npad, P::CDF0, j, make_float4(nrm[0], nrm[1], sdist, __uint_as_float(paff)));
                        stq(out, npad, P::CDF1, j, make_float4(rvel[0], rvel[1], 0.f, 0.f));
                    }
                    ststamp<D>(out, npad, j, epoch);
                }
                if constexpr (G2P_BIN) {
                    if (d.bin_next) {
                        d.cellid[j] = cell_entry;
                        if (moved) d.block_dirty[b] = epoch + 1u;   // b's previous run changes (every writer stores the same value)
                    }
                }
                if (is_mover) {
                    const uint32_t arr_cid = cell_of(cell_entry);
                    if (mv_prev < BLK_ARR) d.blk_arr[(size_t)(arr_cid >> 6) * BLK_ARR + mv_prev] = j;
                    else {   // (more than BLK_ARR arrivals in one block: its cell's list; the index pinned like block_acc's above)
                        uint32_t jj = j;
                        if constexpr (npass <= 2u) asm volatile("" : "+v"(jj));
                        d.mv_next[jj] = atomicExch(&d.cell_head[arr_cid], j + 1u);
                    }
                }
            }  // mine
            if constexpr (G2P_BIN) {
                // grid.wgsl:300-320: a block that holds particles in the next substep and its "+" neighbours are active in it: stamp
                // stores through the links requested above (the first is b itself), once per wave and block
                if (d.bin_next && b != stamped && __ballot(stays) != 0ull) {
                    stamped = b;
                    if (tid < NN) {
                        // (the ids staged for the particles that leave b: its first 2^D are b + {0,1}^D, all active while b holds particles)
                        const uint32_t lk_p = s_nbr[tid];
                        // (a "+" neighbour of a particle-bearing block is always active, so its id is among the staged ones; should one ever
                        // be missing the run says so — ERRBIT_HANDOVER -> wgs_sync — rather than carry a second copy of the insertion code)
                        if (lk_p != NONE) d.block_stamp[lk_p] = epoch + 1u;
                        else if (block_in_key_range<D>(bc)) atomicOr(&d.counters[CTR_ERRORS], ERRBIT_HANDOVER);
                    }
                }
            }
            G2P_PROF(5)
        }  // distinct blocks
    }  // passes of the run
    if constexpr (G2P_CMODE != 2) break;
    run += G2P_GX >> 3;
    }  // runs
    G2P_PROF_LIST(5, wall_clock64())
    G2P_PROF_LIST(1, prof_visits)
