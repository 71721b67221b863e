// p2g_body.inc — the body of the P2G kernels (see kernels_transfer.h), included textually so that the two-body launch
// (k_p2g_pair) compiles exactly the code of the single-body kernels. Expects in scope: d, side, filter, epoch, the
// shared arrays, Cfg / BW / BS / TW / TILE / NT / SLOTS / ROW / KS / NQ / IMPQ, and the macros P2G_CPIC, P2G_TWOWAY,
// P2G_PCDF, P2G_HANDOVER (the slab is handed to grid-update waves of the same launch), P2G_GUESTS_INLAUNCH (pack waves of the
// same launch copy guests' records: the prologue's cdf quads are written through), P2G_BLK, P2G_NBLK (workgroup index
// and count of this body).
    const float *in = d.buf[side];
    const uint32_t npad = d.npad;
    const float h = d.h, inv_h = d.inv_h;
    const int tid0 = threadIdx.x;
    const int sz = D == 3 ? (tid0 >> 6) : 0;  // wave-uniform

    const bool pcdf_thru = P2G_PCDF && pcdf_waves_on(d, epoch, (uint32_t)Cfg::NW);   // (the listed blocks' particle cdf comes from prologue waves of this launch)
    bool s_pcdf_timed_out = false;   // (thread 0's: a wait for the prologue waves timed out in this workgroup — its later blocks do not wait again)
    // (two-way coupling: what an incompatible particle-node pair needs of its collider — velocity_at_point and the lever arm — from LDS:
    // from global memory every such pair was a round trip inside the accumulation loop, and a block next to a collider has hundreds)
    if constexpr (P2G_TWOWAY) {
        for (uint32_t i = (uint32_t)tid0; i < min(d.n_colliders, 16u) * 9u; i += (uint32_t)NT)
            reinterpret_cast<float *>(s_colm)[i] = reinterpret_cast<const float *>(&d.colliders[i / 9u].linvel)[i % 9u];   // (linvel, angvel, com: nine consecutive floats)
        __syncthreads();
    }
    // slab position -> tile node of the entries this thread stores at the end of every block (layout.h): fetched once
    int tmap[(TILE + NT - 1) / NT];
#pragma unroll
    for (int kk = 0; kk < (TILE + NT - 1) / NT; kk++) tmap[kk] = tid0 + kk * NT < TILE ? (int)g_slab_tile_map.t[tid0 + kk * NT] : 0;
    // filter 2 walks the (short) list of blocks near a collider, the others the active list
    // (the near-collider blocks are on eight lists, one per XCD = P2G_BLK & 7; P2G_NBLK is a multiple of 8)
    uint32_t pending = NONE;   // P2G_HANDOVER: block whose slab stores are in flight and whose word is still to be published
    const uint32_t B = min(d.counters[filter == 2 ? ctr_ncpic(P2G_BLK & 7u, epoch) : (uint32_t)CTR_NBLOCKS], d.cap);
    for (uint32_t a = filter == 2 ? P2G_BLK >> 3 : P2G_BLK; a < B; a += filter == 2 ? P2G_NBLK >> 3 : P2G_NBLK) {
        // (the thread index is pinned once per block: every address or LDS offset that is the thread's part of an index would otherwise
        // be computed once, held for the whole launch — in scratch, for want of registers — and fetched back behind a full wait)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int cell = tid & 63;
        int lc[3];
        lc[0] = cell & (BW - 1);
        lc[1] = (cell >> BS) & (BW - 1);
        lc[2] = D == 3 ? (cell >> (2 * BS)) : 0;
        const int tnode0 = lc[0] + TW * lc[1] + (D == 3 ? TW * TW * (lc[2] + sz) : 0);  // tile node of (sx,sy) = (0,0)
        P2G_PROF(0)
        // the active list carries what this body needs of a block (id, key, count, class) and the cells' runs by LIST index:
        // one round trip; the near-collider lists hold block ids: two.
        // (Every variable is defined on every path and the skip decision is one flag: with `uint32_t b, cnt, cs, cn;`
        // assigned in the two branches and `continue`s between the assignments, hipcc 7.2 merged the skip path's undefined
        // `cs` into the path that proceeds — k_p2g<3,false> with filter 1 then read stale cell runs.)
        uint32_t b = 0u, cnt = 0u, cs = 0u, cn = 0u, key = 0u;
        bool skip = false;
        bool direct = false;   // the runs are runs of the buffer itself: no gather through perm (layout.h CELL_DIRECT; workgroup-uniform)
        if (filter == 2) {
            b = d.cpic_list[(size_t)(P2G_BLK & 7u) * d.cap + a];
            cnt = d.block_count[b];
            key = d.block_key[b];
            cs = d.cell_start[b * NPB + cell];
            cn = d.cell_cursor[b * NPB + cell] - cs;
        } else {
            const uint4 info = d.act_info[a];
            const uint2 cr = d.act_cells[(size_t)a * NPB + cell];
            b = info.x;
            key = info.y;
            cnt = info.z;
            cs = cr.x;
            cn = cr.y - cr.x;
            direct = (info.w & CELL_DIRECT) != 0u;
            if (filter == 1) skip = d.listed_in_perm ? (info.w & CELL_LISTED) != 0u : d.block_cpic[b] != 0u;   // the other body's
        }
        if (layer_sel != 0u) {   // (one slab of a decomposition: the boundary layers and the others are two launches)
            int kb[3] = {0, 0, 0};
            unpack_key<D>(key, kb);
            if (shard_boundary_layer(d, kb[0]) != (layer_sel == 1u)) skip = true;
        }
        if constexpr (P2G_HANDOVER) {
            // (a block without particles has no slab to wait for; its word is published all the same, so that a grid-update
            // wave can never wait for a block this body passed over)
            if (cnt == 0 && filter != 2 && tid == 0) __hip_atomic_store(&d.slab_epoch[b], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (cnt == 0 || skip) continue;  // (no particles: its slab is never read)
#ifdef WGS_ABLATE
        if (!P2G_CPIC) { P2G_PROF(6) }   // (plain body: the block's record and runs are in)
#endif
        int bc[3] = {0, 0, 0};
        unpack_key<D>(key, bc);
        __syncthreads();  // previous block fully consumed
        if constexpr (P2G_PCDF) {
          stage_node_cdf_tile<D, NT>(d, b, s_ncdf, tid);   // (for the particle cdf below and for the affinities of the target nodes further down)
          bool own_prologue = !pcdf_thru;
          if (pcdf_thru) {   // (uniform over the launch) the prologue waves of this launch take the particle cdf: kernels_transfer.h pcdf_waves
            if (tid == 0) {
                const unsigned long long t_start = wall_clock64();
                uint32_t gave_up = 0u;
                while (__hip_atomic_load(&d.pcdf_done[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != cnt) {
                    // (0.2 s at 100 MHz, once per launch and workgroup: a visit list that lost entries, or prologue workgroups that were
                    // not dispatched ahead of this one — reported under a bit of its own, never a hang, and never stale quads: the
                    // workgroup then computes the block's particle cdf itself, below; what a late wave still writes is the same bytes)
                    if (s_pcdf_timed_out || wall_clock64() - t_start > 20000000ull) {
                        atomicOr(&d.counters[CTR_ERRORS], ERRBIT_PCDF);
                        gave_up = 1u;
                        s_pcdf_timed_out = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
                s_cs[0] = gave_up;   // (the runs are staged after the prologue: the slot is free)
            }
            __syncthreads();
            own_prologue = s_cs[0] != 0u;
            __syncthreads();
          }
          if (own_prologue) {
            __syncthreads();
            const uint32_t bstart = d.block_start[b];
            // (rolling prefetch, one copy of the code: the sort entry of the particle after the next one and the state of the next one are
            // in flight while this one is computed — the chain sort entry -> state -> cdf was paid once per particle, three to six
            // times per thread of a full block)
            {
                const uint32_t jend = bstart + cnt;
                uint32_t j = bstart + (uint32_t)tid;
                uint32_t src0 = j < jend ? d.perm[j] : NONE;
                uint32_t src1 = j + (uint32_t)NT < jend ? d.perm[j + (uint32_t)NT] : NONE;
                ParticleCdfIn in0 = {make_float4(0.f, 0.f, 0.f, 0.f), 0u, 0u};
                if (src0 != NONE) in0 = particle_cdf_fetch<D>(d, d.buf[side], src0);
#pragma unroll 1
                while (src0 != NONE) {
                    const uint32_t src2 = j + 2u * (uint32_t)NT < jend ? d.perm[j + 2u * (uint32_t)NT] : NONE;
                    ParticleCdfIn in1 = {make_float4(0.f, 0.f, 0.f, 0.f), 0u, 0u};
                    if (src1 != NONE) in1 = particle_cdf_fetch<D>(d, d.buf[side], src1);
                    particle_cdf_update<D, P2G_GUESTS_INLAUNCH>(d, d.buf[side], src0, in0, s_ncdf, bc, epoch);
                    src0 = src1;
                    in0 = in1;
                    src1 = src2;
                    j += (uint32_t)NT;
                }
            }
            __threadfence_block();
            __syncthreads();  // the affinities written above are fetched below by other threads of the workgroup
          }
        }
        if (P2G_CPIC) { P2G_PROF(6) }  // (CPIC body: particle cdf prologue done)
        if (tid < NPB) {
            s_cs[cell] = cs;
            s_cn[cell] = cn;
        }
        for (int n = cell; n < TILE; n += 64) s_tile[sz][n] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (P2G_TWOWAY) {
            for (int n = cell; n < TILE; n += 64)
                for (int q = 0; q < IMPQ; q++) s_imp[sz][q][n] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const uint32_t maxc = wave_max_u32(cn);
#ifdef WGS_ABLATE
        if (!P2G_CPIC && maxc != 0xfffffffeu) { P2G_PROF(7) }   // (plain body: runs in LDS, tile zeroed, longest run known)
#endif
        float cpos[D];
#pragma unroll
        for (int k = 0; k < D; k++) cpos[k] = (float)(bc[k] * BW + lc[k]) * h;
        uint32_t naff[Cfg::NSXY];
        unsigned long long ncol = 0ull;  // closest collider of the nine nodes: 4 bits each + valid bit at 36 + s
        if constexpr (P2G_CPIC) {  // affinities of this thread's nine target nodes (p2g.wgsl:100-103)
#pragma unroll
            for (int s = 0; s < 9; s++) {
                int t[3] = {lc[0] + s % 3, lc[1] + s / 3, lc[2] + sz};
                int o = (t[0] >= BW ? 1 : 0) | (t[1] >= BW ? 2 : 0) | (t[2] >= BW ? 4 : 0);
                int ln = (t[0] & (BW - 1)) + ((t[1] & (BW - 1)) << BS) + (D == 3 ? ((t[2] & (BW - 1)) << (2 * BS)) : 0);
                if constexpr (P2G_PCDF) {
                    // the prologue staged the node cdfs of the tile (absent neighbours: no affinity, no collider): LDS
                    // instead of 9 x 2 dependent global loads per thread
                    const NodeCdf nc = s_ncdf[tnode0 + (s % 3) + TW * (s / 3)];
                    naff[s] = nc.affinities;
                    if constexpr (P2G_TWOWAY) {
                        if (nc.closest_id < 16u) ncol |= ((unsigned long long)nc.closest_id << (4 * s)) | (1ull << (36 + s));
                    }
                } else {
                    uint32_t nb = d.nbr_plus[b * 8u + o];
                    naff[s] = nb != NONE ? d.node_cdf[(size_t)nb * NPB + ln].affinities : 0u;
                    if constexpr (P2G_TWOWAY) {
                        const uint32_t cl = nb != NONE ? d.node_cdf[(size_t)nb * NPB + ln].closest_id : NONE;
                        if (cl < 16u) ncol |= ((unsigned long long)cl << (4 * s)) | (1ull << (36 + s));
                    }
                }
            }
        }
        if (P2G_CPIC) { P2G_PROF(7) }  // (CPIC body: node affinities in)
        float acc[Cfg::NSXY][D + 1];
#pragma unroll
        for (int s = 0; s < 9; s++)
#pragma unroll
            for (int k = 0; k <= D; k++) acc[s][k] = 0.f;

        // Software-pipelined staging: the particle quads of round r+1 are fetched into registers while
        // round r is being accumulated from LDS, so the HBM latency of a round hides behind the
        // previous round's arithmetic instead of being paid at every barrier.
        // Staging slot sl -> (cell c = sl / J, rank j = sl % J): a cell's J particles are one contiguous
        // 64-byte run of each quad in HBM; in LDS they go to [j][c] (row padded to ROW).
        float4 pre[KS][NQ];
        float4 pre_nrm[P2G_TWOWAY ? KS : 1];
        uint32_t pre_aff[KS];
        bool pre_ok[KS];
        __syncthreads();  // s_cs / s_cn visible
        P2G_PROF(1)
        auto fetch_round = [&](uint32_t r0) {
#pragma unroll
            for (int k = 0; k < KS; k++) {
                const int sl = tid + k * NT;
                pre_ok[k] = false;
                if (sl < SLOTS) {
                    const int c = sl / P2G_J;
                    const uint32_t rank = r0 + (uint32_t)(sl % P2G_J);
                    if (rank < s_cn[c] WGS_ABLATE_AND(!(d.dbg & DBG_ABLATE_P2G_NO_LOADS))) {
                        const uint32_t src = direct ? s_cs[c] + rank : d.perm[s_cs[c] + rank];
                        pre_ok[k] = true;
                        if constexpr (D == 3) {
                            pre[k][0] = ldq(in, npad, Pl<3>::XM, src);
                            pre[k][1] = ldq(in, npad, Pl<3>::CV0, src);
                            pre[k][2] = ldq(in, npad, Pl<3>::CV1, src);
                            pre[k][3] = ldq(in, npad, Pl<3>::CV2, src);
                        } else {
                            pre[k][0] = ldq(in, npad, Pl<2>::XM, src);   // x, y, m, V0
                            pre[k][1] = ldq(in, npad, Pl<2>::CV0, src);
                            pre[k][2] = ldq(in, npad, Pl<2>::CV2, src);  // vx, vy, lambda, mu
                        }
                        if constexpr (P2G_CPIC) {
                            // (written by another workgroup of this launch when it has prologue waves: fetched past this XCD's L2 then)
                            const bool thru = P2G_PCDF && pcdf_thru;
                            const __amdgpu_buffer_rsrc_t pr = particle_rsrc<D>(d.buf[side], npad);
                            const int qa = D == 3 ? (int)Pl<D>::CDF1 : (int)Pl<D>::CDF0;
                            const float4 cd = thru ? ld_agent(pr, quad_off(npad, qa, src)) : ldq(in, npad, qa, src);
                            pre_aff[k] = __float_as_uint(cd.w);
                            if constexpr (P2G_TWOWAY) pre_nrm[k] = D == 3 ? (thru ? ld_agent(pr, quad_off(npad, (int)Pl<D>::CDF0, src)) : ldq(in, npad, Pl<D>::CDF0, src)) : cd;  // cdf normal
                        }
                    }
                }
            }
        };
        fetch_round(0);
        P2G_PROF(2)
        for (uint32_t r0 = 0; r0 < maxc; r0 += P2G_J) {
            __syncthreads();  // previous round consumed
#pragma unroll
            for (int k = 0; k < KS; k++) {
                if (pre_ok[k]) {
                    const int sl = tid + k * NT;
                    const int dst = (sl % P2G_J) * ROW + sl / P2G_J;
                    if constexpr (D == 3) {
                        float4 c2 = pre[k][3];
                        const float m = P2G_TWOWAY ? 1.f : (d.uniform ? d.uni_mass : pre[k][0].w);  // (the two-way path needs the raw velocity too)
                        c2.y *= m; c2.z *= m; c2.w *= m;  // momentum m v
                        s_q[0][dst] = pre[k][0]; s_q[1][dst] = pre[k][1]; s_q[2][dst] = pre[k][2]; s_q[3][dst] = c2;
                    } else {
                        float4 vl = pre[k][2];
                        const float m = P2G_TWOWAY ? 1.f : pre[k][0].z;
                        vl.x *= m; vl.y *= m;
                        s_q[0][dst] = pre[k][0]; s_q[1][dst] = pre[k][1]; s_q[2][dst] = vl;
                    }
                    if constexpr (P2G_CPIC) s_aff[dst] = pre_aff[k];
                    if constexpr (P2G_TWOWAY) s_nrm[dst] = pre_nrm[k];
                }
            }
            __syncthreads();
            if (r0 == 0) { P2G_PROF(3) }
            if (r0 + P2G_J < maxc) fetch_round(r0 + P2G_J);  // in flight during the accumulation below
            const uint32_t jn = (cn > r0 WGS_ABLATE_AND(!(d.dbg & DBG_ABLATE_P2G_NO_ACCUM))) ? min((uint32_t)P2G_J, cn - r0) : 0u;
            for (uint32_t j = 0; j < jn; j++) {
                const int sl = j * ROW + cell;
                float x[D], mv[D], c[D * D], mass;
                if constexpr (D == 3) {
                    const float4 xm = s_q[0][sl], c0 = s_q[1][sl], c1 = s_q[2][sl], c2 = s_q[3][sl];
                    x[0] = xm.x; x[1] = xm.y; x[2] = xm.z; mass = d.uniform ? d.uni_mass : xm.w;  // (uniform mode: XM.w holds F[8])
                    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w;
                    c[4] = c1.x; c[5] = c1.y; c[6] = c1.z; c[7] = c1.w; c[8] = c2.x;
                    mv[0] = c2.y; mv[1] = c2.z; mv[2] = c2.w;
                } else {
                    const float4 xm = s_q[0][sl], c0 = s_q[1][sl], vl = s_q[2][sl];
                    x[0] = xm.x; x[1] = xm.y; mass = xm.z;
                    c[0] = c0.x; c[1] = c0.y; c[2] = c0.z; c[3] = c0.w;
                    mv[0] = vl.x; mv[1] = vl.y;
                }
                uint32_t paff = 0u;
                if constexpr (P2G_CPIC) paff = s_aff[sl];
                float pv[D], pn[D];  // raw particle velocity and cdf normal (two-way coupling)
                if constexpr (P2G_TWOWAY) {
                    const float4 nq = s_nrm[sl];
                    pn[0] = nq.x; pn[1] = nq.y;
                    if constexpr (D == 3) pn[2] = nq.z;
#pragma unroll
                    for (int k = 0; k < D; k++) {
                        pv[k] = mv[k];
                        mv[k] = mv[k] * mass;
                    }
                }
                // p2g.wgsl:176-198: ref = assoc_node - x ; w = eval_all(-ref / h) ; dpt = ref + shift * h
                float ref[D], wx[3], wy[3];
#pragma unroll
                for (int k = 0; k < D; k++) ref[k] = cpos[k] - x[k];
                eval_all(-ref[0] * inv_h, wx);
                eval_all(-ref[1] * inv_h, wy);
                float wzs = 1.f;
                float base[D];  // C[:, 2] * dz + m v
                if constexpr (D == 3) {
                    float wz[3];
                    eval_all(-ref[2] * inv_h, wz);
                    wzs = sz == 0 ? wz[0] : (sz == 1 ? wz[1] : wz[2]);
                    const float dz = ref[2] + (float)sz * h;
#pragma unroll
                    for (int k = 0; k < 3; k++) base[k] = c[6 + k] * dz + mv[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 2; k++) base[k] = mv[k];
                }
#pragma unroll
                for (int sy = 0; sy < 3; sy++) {
                    const float dy = ref[1] + (float)sy * h;
                    const float wyz = wy[sy] * wzs;
                    float py[D];
#pragma unroll
                    for (int k = 0; k < D; k++) py[k] = c[D + k] * dy + base[k];
#pragma unroll
                    for (int sx = 0; sx < 3; sx++) {
                        const int s = sx + 3 * sy;
                        if constexpr (P2G_CPIC) {
                            // p2g.wgsl:200-228: incompatible pairs transfer nothing to the grid (their momentum
                            // becomes an impulse on the rigid body: two-way coupling, SURVEY §8 f1)
                            if (!affinities_are_compatible(naff[s], paff)) {
                                if constexpr (P2G_TWOWAY) {
                                    if ((ncol >> (36 + s)) & 1ull) {  // p2g.wgsl:203-224
                                        const ColliderMotion &cl = s_colm[(uint32_t)(ncol >> (4 * s)) & 15u];
                                        const float wgt = wx[sx] * wyz;
                                        float dpt[3] = {ref[0] + (float)sx * h, dy, 0.f}, cc[3] = {0.f, 0.f, 0.f};
                                        if constexpr (D == 3) dpt[2] = ref[2] + (float)sz * h;
#pragma unroll
                                        for (int k = 0; k < D; k++) cc[k] = dpt[k] + x[k];  // cell_center
                                        float bv[D], rel[D], prj[D], dimp[3] = {0.f, 0.f, 0.f}, lever[3] = {0.f, 0.f, 0.f};
                                        velocity_at_point<D>(cl, cc, bv);
#pragma unroll
                                        for (int k = 0; k < D; k++) rel[k] = pv[k] - bv[k];
                                        project_velocity<D>(rel, pn, prj);
#pragma unroll
                                        for (int k = 0; k < D; k++) {
                                            const float ghost = bv[k] + prj[k];
                                            dimp[k] = (pv[k] - ghost) * (wgt * mass);
                                            lever[k] = cl.com[k] - cc[k];
                                        }
                                        const int node = tnode0 + sx + TW * sy;
                                        if constexpr (D == 3) {
                                            float4 a = s_imp[sz][0][node], bq = s_imp[sz][1][node];
                                            a.x += dimp[0]; a.y += dimp[1]; a.z += dimp[2];
                                            bq.x += dimp[1] * lever[2] - dimp[2] * lever[1];
                                            bq.y += dimp[2] * lever[0] - dimp[0] * lever[2];
                                            bq.z += dimp[0] * lever[1] - dimp[1] * lever[0];
                                            s_imp[sz][0][node] = a;
                                            s_imp[sz][1][node] = bq;
                                        } else {
                                            float4 a = s_imp[sz][0][node];
                                            a.x += dimp[0]; a.y += dimp[1];
                                            a.z += dimp[0] * lever[1] + dimp[1] * (-lever[0]);
                                            s_imp[sz][0][node] = a;
                                        }
                                        // lanes own distinct nodes within one (sx, sy) phase; keep the phases in order
                                        asm volatile("" ::: "memory");
                                    }
                                }
                                continue;
                            }
                        }
                        const float dx = ref[0] + (float)sx * h;
                        const float w = wx[sx] * wyz;
#pragma unroll
                        for (int k = 0; k < D; k++) acc[s][k] += (c[k] * dx + py[k]) * w;
                        acc[s][D] += mass * w;
                    }
                }
            }
        }
        P2G_PROF(4)
        // Per-wave tile: in phase (sx, sy) every lane (cell) owns a distinct node, so a plain float4
        // read-add-write is race-free inside the wave and the LDS executes a wave's accesses in order.
        // The asm memory clobbers stop hipcc from hoisting a later phase's load above an earlier phase's
        // store (legal for one thread, wrong across lanes).
        {
            asm volatile("; WGS_TILE_PHASE_END" ::: "memory");  // (opens the first phase)
#pragma unroll
            for (int s = 0; s < 9; s++) {
                float4 *p = &s_tile[sz][tnode0 + (s % 3) + TW * (s / 3)];   // (immediate offsets from one base)
                float4 v = *p;
                v.x += acc[s][0]; v.y += acc[s][1]; v.z += acc[s][2];
                if constexpr (D == 3) v.w += acc[s][3];
                *p = v;
                // (compiler barrier; the marker survives into the ISA, where tests/test_isa_order.py checks that no
                // load of a later phase has been hoisted above this phase's store)
                asm volatile("; WGS_TILE_PHASE_END" ::: "memory");
            }
        }
        if constexpr (P2G_HANDOVER) {
            // The previous block's slab is complete once every thread's write-through stores have been acknowledged: then,
            // and only then, the block's word tells the grid-update waves of this launch (gu_waves) that they may gather
            // from it. Waiting HERE costs nothing — those stores were issued a whole block ago, before every load of this
            // block, and the counter retires in order — where a wait right behind the stores put their latency on the
            // workgroup's critical path (C5: P2G + grid update 405 -> 461 us).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if constexpr (P2G_HANDOVER) {
            if (tid == 0 && pending != NONE) __hip_atomic_store(&d.slab_epoch[pending], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // combine the sz tiles in a fixed order; one coalesced slab store per node
        // (slab position pn <- tile node n: the slab is stored by regions, layout.h; consecutive threads store consecutively)
#pragma unroll
        for (int kk = 0; kk < (TILE + NT - 1) / NT; kk++) {
            const int pn = tid + kk * NT;
            if (pn >= TILE) break;
            const int n = tmap[kk];
            float4 sum = s_tile[0][n];
#pragma unroll
            for (int w = 1; w < Cfg::NW; w++) {
                const float4 p = s_tile[w][n];
                sum.x += p.x; sum.y += p.y; sum.z += p.z; sum.w += p.w;
            }
            if constexpr (P2G_HANDOVER) st_agent(slab_rsrc(&d.slab[(size_t)__builtin_amdgcn_readfirstlane((int)b) * TILE], TILE * 16u), (uint32_t)pn * 16u, sum);   // (written through: read by another XCD in this launch)
            else d.slab[(size_t)b * TILE + pn] = sum;
            if constexpr (P2G_TWOWAY) {
#pragma unroll
                for (int q = 0; q < IMPQ; q++) {
                    const int nl = tmap[kk];
                    float4 is = s_imp[0][q][nl];
#pragma unroll
                    for (int w = 1; w < Cfg::NW; w++) {
                        const float4 p = s_imp[w][q][nl];
                        is.x += p.x; is.y += p.y; is.z += p.z;
                    }
                    if constexpr (P2G_HANDOVER) st_agent(slab_rsrc(&d.imp_slab[(size_t)__builtin_amdgcn_readfirstlane((int)b) * TILE * IMPQ], TILE * IMPQ * 16u), (uint32_t)(pn * IMPQ + q) * 16u, is);
                    else d.imp_slab[((size_t)b * TILE + pn) * IMPQ + q] = is;
                }
            }
        }
        if constexpr (P2G_HANDOVER) pending = b;   // published one block later, or at the end (below)
        P2G_PROF(5)
    }
    if constexpr (P2G_HANDOVER) {
        if (pending != NONE) {   // (workgroup-uniform)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid0 == 0) __hip_atomic_store(&d.slab_epoch[pending], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
