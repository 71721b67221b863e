// host_substep.inc — one substep on the data's stream: the tunables of the launch shapes, the launch ladders (which
// instantiation a decided shape means), the launch plans (which shape a substep takes: plan_sort, plan_p2g, plan_g2p) and
// the stages that string them together: begin_substep decides, once, everything the substep's launches share; enqueue_sort,
// enqueue_p2g and enqueue_finish launch. Everything that decides WHAT is launched lives here; entry points only run the
// stages (wgs_step all four, the phases of host_sharded.inc begin + sort + P2G | finish) or call enqueue_bodies.

namespace {

wgs_status allreduce_impulses(wgs_data *d);  // host_sharded.inc
void launch_bodies_integrate(wgs_data *d);   // behind the stages
void launch_grid_walls(wgs_data *d);         // capi_walls.inc
void launch_grid_forces(wgs_data *d);        // capi_forces.inc
wgs_status fire_emitters(wgs_data *d, bool timed);   // capi_emit.inc (wgs_step, in front of begin_substep)
wgs_status fire_sinks(wgs_data *d, bool timed);      // capi_remove.inc (wgs_step, in front of fire_emitters)

#ifndef WGS_PCDF_WAVES_MAX_VISITS
#define WGS_PCDF_WAVES_MAX_VISITS 256
#endif
constexpr uint32_t PCDF_WAVES_MAX_VISITS = WGS_PCDF_WAVES_MAX_VISITS;   // per XCD list: above, the prologue waves would be a round of work in front of the launch, not a use of idle CUs
constexpr uint32_t P2G_SMALL_BUDGET_MIN_PARTICLES = 600000;  // one-way CPIC P2G body at 168 VGPRs from this size on
#ifndef WGS_REGROUP_ROUNDS
#define WGS_REGROUP_ROUNDS 4u
#endif
#ifndef WGS_GU_WG_PER_CU
#define WGS_GU_WG_PER_CU 8
#endif
#ifndef WGS_PLASTIC_WPE_DENSE
#define WGS_PLASTIC_WPE_DENSE 2
#endif
#ifndef WGS_PLASTIC_WPE
#define WGS_PLASTIC_WPE G2P_WAVES_PER_EU
#endif
constexpr uint32_t P2G_PAIR_MIN_BLOCKS = 8;  // near-collider blocks from which P2G runs both bodies in one launch

// ---- launch ladders of the stages: each takes the shape a plan decided and lists exactly the instantiations that exist.
// (Templates on the dimension, like the stages themselves: they are instantiated where wgs_step reaches them, which keeps the
// kernels in the code object in the order of their first use — placement alone moves a kernel by a few percent, DESIGN 9.7.)

// pack waves of a slab with neighbours: one per interface block as the host last saw the grid (a face holds a fraction of the
// active blocks), plus a few for the guests
struct PackWaves {
    uint32_t blocks, guests;
};
PackWaves pack_waves(const wgs_data *d) {
    return {std::max(64u, std::min(2048u, d->seen.nblocks ? d->seen.nblocks : 2048u)), std::max(1u, std::min(64u, (2u * d->link->mig_cap + 63u) / 64u))};
}

// launch 2 of the sort (kernels_sort.h): CDF = the node cdfs and block classes ride in it; SUMM = blocks share node-cdf summaries
template <int DIM> void launch_regroup(const Dev &dev, hipStream_t s, dim3 g, int side, uint32_t epoch, uint32_t nscan, int have_old, bool cdf, bool summ) {
    const dim3 b(SORT_THREADS);
    if (cdf && dev.sharded && summ) hipLaunchKernelGGL((k_regroup<DIM, true, true, true>), g, b, 0, s, dev, side, epoch, nscan, have_old);
    else if (cdf && dev.sharded) hipLaunchKernelGGL((k_regroup<DIM, true, true>), g, b, 0, s, dev, side, epoch, nscan, have_old);
    else if (cdf && summ) hipLaunchKernelGGL((k_regroup<DIM, true, false, true>), g, b, 0, s, dev, side, epoch, nscan, have_old);
    else if (cdf) hipLaunchKernelGGL((k_regroup<DIM, true, false>), g, b, 0, s, dev, side, epoch, nscan, have_old);
    else if (dev.sharded) hipLaunchKernelGGL((k_regroup<DIM, false, true>), g, b, 0, s, dev, side, epoch, nscan, have_old);
    else hipLaunchKernelGGL((k_regroup<DIM, false, false>), g, b, 0, s, dev, side, epoch, nscan, have_old);
}

enum class P2gShape {
    plain,       // no collider: the plain body
    separate,    // the plain body, then the CPIC body (particle cdf in its prologue) in a launch of its own
    cpic_first,  // the CPIC body first, then the plain body with the grid update riding in it
    pair,        // both bodies in one launch (k_p2g_pair)
};
struct P2gLaunch {
    P2gShape shape;
    bool two_way;       // the two-way CPIC body
    bool small_budget;  // pair, one-way: the CPIC body cut to 168 VGPRs
    int gu;             // what rides in the last launch (kernels_transfer.h GU): 0 nothing, 2 the grid update, 3 a slab's pack waves + interior update
    uint32_t wgs;       // workgroups per body
    uint32_t ride;      // workgroups behind the P2G workgroups of the last launch: npack + the grid update's
    uint32_t npack, npack_blk, layer_sel;
    uint32_t npro;      // prologue workgroups (kernels_transfer.h pcdf_waves)
};

template <int DIM, bool TW, int WPE> void launch_p2g_pair(Dev &dev, hipStream_t s, int side, uint32_t epoch, const P2gLaunch &p) {
    const dim3 g(p.npro + 2u * p.wgs + p.ride), b(P2GCfg<DIM>::NW * 64);
    dev.pcdf_waves = p.npro;
    if (p.gu == 2) hipLaunchKernelGGL((k_p2g_pair<DIM, TW, WPE, 2>), g, b, 0, s, dev, side, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, p.npro);
    else if (p.gu == 3) hipLaunchKernelGGL((k_p2g_pair<DIM, TW, WPE, 3>), g, b, 0, s, dev, side, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, p.npro);
    else hipLaunchKernelGGL((k_p2g_pair<DIM, TW, WPE, 0>), g, b, 0, s, dev, side, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, p.npro);
    dev.pcdf_waves = 0u;
}

// the last P2G launch of the substep, with what rides behind its workgroups
template <int DIM, bool CP, bool TW, bool PC> void launch_p2g_last(Dev &dev, hipStream_t s, int side, int filter, uint32_t epoch, const P2gLaunch &p) {
    const uint32_t npro = PC ? p.npro : 0u;
    const dim3 g(npro + p.wgs + p.ride), b(P2GCfg<DIM>::NW * 64);
    dev.pcdf_waves = npro;
    if (p.gu == 2) hipLaunchKernelGGL((k_p2g<DIM, CP, TW, PC, 2>), g, b, 0, s, dev, side, filter, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, npro);
    else if (p.gu == 3) hipLaunchKernelGGL((k_p2g<DIM, CP, TW, PC, 3>), g, b, 0, s, dev, side, filter, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, npro);
    else hipLaunchKernelGGL((k_p2g<DIM, CP, TW, PC, 0>), g, b, 0, s, dev, side, filter, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, npro);
    dev.pcdf_waves = 0u;
}

template <int DIM> void launch_p2g(Dev &dev, hipStream_t s, int side, uint32_t epoch, const P2gLaunch &p) {
    const dim3 g(p.wgs), b(P2GCfg<DIM>::NW * 64);
    switch (p.shape) {
        case P2gShape::pair:
            if (p.two_way) launch_p2g_pair<DIM, true, 1>(dev, s, side, epoch, p);
            else if (p.small_budget) launch_p2g_pair<DIM, false, 3>(dev, s, side, epoch, p);
            else launch_p2g_pair<DIM, false, 1>(dev, s, side, epoch, p);
            break;
        case P2gShape::cpic_first:
            dev.pcdf_waves = p.npro;
            hipLaunchKernelGGL((k_p2g<DIM, true, true, true, 1>), dim3(p.npro + p.wgs), b, 0, s, dev, side, 2, epoch, p.wgs, 0u, 0u, p.layer_sel, p.npro);
            dev.pcdf_waves = 0u;
            hipLaunchKernelGGL((k_p2g<DIM, false, false, false, 2, true>), dim3(p.wgs + p.ride), b, 0, s, dev, side, 1, epoch, p.wgs, p.npack, p.npack_blk, p.layer_sel, 0u);
            break;
        case P2gShape::separate:
            // (the first of the two launches hands its slabs over like the last one when anything rides in that one)
            if (p.gu != 0) hipLaunchKernelGGL((k_p2g<DIM, false, false, false, 1>), g, b, 0, s, dev, side, 1, epoch, p.wgs, 0u, 0u, p.layer_sel, 0u);
            else hipLaunchKernelGGL((k_p2g<DIM, false>), g, b, 0, s, dev, side, 1, epoch, p.wgs, 0u, 0u, p.layer_sel, 0u);
            // near-collider list: particle cdf in the prologue (the node cdfs are complete: k_setup_scatter<CDF>, or
            // k_cdf after k_p2g_cdf with mesh colliders), then the CPIC transfer
            if (p.two_way) launch_p2g_last<DIM, true, true, true>(dev, s, side, 2, epoch, p);
            else launch_p2g_last<DIM, true, false, true>(dev, s, side, 2, epoch, p);
            break;
        case P2gShape::plain:
            launch_p2g_last<DIM, false, false, false>(dev, s, side, 0, epoch, p);
            break;
    }
}

// PHASE 0: every block of single-domain data; 3: a slab's blocks after the exchange (iface_only: the interior's rode in P2G)
template <int DIM> void launch_grid_update(const Dev &dev, hipStream_t s, dim3 g, uint32_t epoch, bool slab, bool two_way, uint32_t iface_only) {
    if (!slab && two_way) hipLaunchKernelGGL((k_grid_update<DIM, 0, true>), g, dim3(256), 0, s, dev, epoch, 0u);
    else if (!slab) hipLaunchKernelGGL((k_grid_update<DIM, 0>), g, dim3(256), 0, s, dev, epoch, 0u);
    else if (two_way) hipLaunchKernelGGL((k_grid_update<DIM, 3, true>), g, dim3(256), 0, s, dev, epoch, iface_only);
    else hipLaunchKernelGGL((k_grid_update<DIM, 3>), g, dim3(256), 0, s, dev, epoch, iface_only);
}

enum class G2pShape {
    single,        // no collider: one launch
    two_launches,  // the plain body, then the CPIC body in a launch of its own
    pair,          // both bodies in one launch (k_g2p_pair)
    pair_dense,    // ... in the spill-free plastic variant
};
struct G2pLaunch {
    G2pShape shape;
    bool shard;
    uint32_t g;      // main-body waves: one per `npass` chunks of 64 sorted particles, a multiple of 8 (XCD-aware mapping)
    uint32_t nlist;  // list waves per XCD of the CPIC body (8 x nlist in all)
};

// (the decomposition is a template parameter of the fused G2P: kernels_transfer.h; BIN: not the plastic variants)
template <int DIM, int MODEL, bool PL, int NP, class Mark>
void launch_g2p_shape(const Dev &dev, hipStream_t s, int side, uint32_t epoch, const G2pLaunch &p, const Mark &mark) {
    constexpr int WPE = PL ? WGS_PLASTIC_WPE : G2P_WAVES_PER_EU, WPE_DENSE = PL ? WGS_PLASTIC_WPE_DENSE : G2P_WAVES_PER_EU;
    // (per-particle models exist on single-domain data only — wgs_set_particle_models refuses slabs —: no slab instantiation of MODEL 3)
    // (likewise the snow rule, MODEL 4: wgs_set_plasticity_model refuses slabs)
    constexpr bool SH = MODEL != 3 && MODEL != 4;
    const dim3 g(p.g), pg(p.g + 8u * p.nlist), t(G2P_THREADS);
    switch (p.shape) {
        case G2pShape::pair_dense:
            if (p.shard) hipLaunchKernelGGL((k_g2p_pair<DIM, MODEL, PL, WPE_DENSE, NP, SH, !PL>), pg, t, 0, s, dev, side, epoch, p.g, p.nlist);
            else hipLaunchKernelGGL((k_g2p_pair<DIM, MODEL, PL, WPE_DENSE, NP, false, !PL>), pg, t, 0, s, dev, side, epoch, p.g, p.nlist);
            break;
        case G2pShape::pair:
            if (p.shard) hipLaunchKernelGGL((k_g2p_pair<DIM, MODEL, PL, WPE, NP, SH, !PL>), pg, t, 0, s, dev, side, epoch, p.g, p.nlist);
            else hipLaunchKernelGGL((k_g2p_pair<DIM, MODEL, PL, WPE, NP, false, !PL>), pg, t, 0, s, dev, side, epoch, p.g, p.nlist);
            break;
        case G2pShape::two_launches:
            hipLaunchKernelGGL((k_g2p_update<DIM, MODEL, PL, 1, NP, false, !PL>), g, t, 0, s, dev, side, epoch);
            mark(6);
            hipLaunchKernelGGL((k_g2p_update<DIM, MODEL, PL, 2, 1, false, !PL>), dim3(8u * p.nlist), t, 0, s, dev, side, epoch);
            break;
        case G2pShape::single:
            if (p.shard) hipLaunchKernelGGL((k_g2p_update<DIM, MODEL, PL, 0, NP, SH, !PL>), g, t, 0, s, dev, side, epoch);
            else hipLaunchKernelGGL((k_g2p_update<DIM, MODEL, PL, 0, NP, false, !PL>), g, t, 0, s, dev, side, epoch);
            break;
    }
}

template <int DIM, int MODEL, bool PL, class Mark>
void launch_g2p_model(const Dev &dev, hipStream_t s, int side, uint32_t epoch, const G2pLaunch &p, const Mark &mark) {
    if (dev.g2p_npass == (uint32_t)G2P_MANY_PASSES) launch_g2p_shape<DIM, MODEL, PL, G2P_MANY_PASSES>(dev, s, side, epoch, p, mark);
    else if (dev.g2p_npass == 2u) launch_g2p_shape<DIM, MODEL, PL, 2>(dev, s, side, epoch, p, mark);
    else launch_g2p_shape<DIM, MODEL, PL, 1>(dev, s, side, epoch, p, mark);
}

// The G2P variant of the data, in the order of the ladders below (which is the order of their kernels in the code object).
// (the fluid exists without plastic state only — wgs_set_constitutive_model refuses it on such data — and comes last: the
// instantiations of the other models keep their places in the code object)
// (a table of per-particle models — Dev::pmodel, likewise without plastic state and on single-domain data only — behind the fluid)
// (snow — the corotated plastic variant under the other plasticity rule, wgs_set_plasticity_model; single-domain data with plastic
// state only — behind them all, and its kernels behind every kernel of the library: launch_g2p_snow, capi_plasticity.inc)
enum class G2pVariant { corotated, corotated_plastic, neo_hookean, neo_hookean_plastic, fluid, per_particle, snow };
G2pVariant g2p_variant(const Dev &dev, bool plastic, int32_t plasticity = WGS_PLASTICITY_DRUCKER_PRAGER) {
    // (WGS_PLASTICITY_SNOW is only ever set under WGS_MODEL_COROTATED, and plastic data carries no table: wgs_set_plasticity_model)
    if (plastic && plasticity == WGS_PLASTICITY_SNOW) return G2pVariant::snow;
    if (dev.pmodel[0]) return G2pVariant::per_particle;
    if (dev.model == WGS_MODEL_FLUID) return G2pVariant::fluid;
    if (dev.model == WGS_MODEL_NEO_HOOKEAN) return plastic ? G2pVariant::neo_hookean_plastic : G2pVariant::neo_hookean;
    return plastic ? G2pVariant::corotated_plastic : G2pVariant::corotated;
}

struct Mark;
void launch_g2p_snow(const Dev &dev, hipStream_t s, int side, uint32_t epoch, const G2pLaunch &p, const Mark &mark);   // capi_plasticity.inc

// the fused G2P; `mark(6)` between the two launches of that shape
template <int DIM, class Mark> void launch_g2p(const Dev &dev, hipStream_t s, int side, uint32_t epoch, bool plastic, int32_t plasticity, const G2pLaunch &p, const Mark &mark) {
    switch (g2p_variant(dev, plastic, plasticity)) {
        case G2pVariant::corotated: launch_g2p_model<DIM, 0, false>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::corotated_plastic: launch_g2p_model<DIM, 0, true>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::neo_hookean: launch_g2p_model<DIM, 1, false>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::neo_hookean_plastic: launch_g2p_model<DIM, 1, true>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::fluid: launch_g2p_model<DIM, 2, false>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::per_particle: launch_g2p_model<DIM, 3, false>(dev, s, side, epoch, p, mark); break;
        case G2pVariant::snow: launch_g2p_snow(dev, s, side, epoch, p, mark); break;   // (MODEL 4, instantiated behind every other kernel)
    }
}

// (a slab has no per-particle models — wgs_set_particle_models refuses it —: no arrivals' kernel of that variant)
template <int DIM> void launch_arrivals(const Dev &dev, hipStream_t s, dim3 g, int side, uint32_t epoch, bool plastic) {
    switch (g2p_variant(dev, plastic)) {
        case G2pVariant::corotated: hipLaunchKernelGGL((k_g2p_arrivals<DIM, 0, false>), g, dim3(256), 0, s, dev, side, epoch); break;
        case G2pVariant::corotated_plastic: hipLaunchKernelGGL((k_g2p_arrivals<DIM, 0, true>), g, dim3(256), 0, s, dev, side, epoch); break;
        case G2pVariant::neo_hookean: hipLaunchKernelGGL((k_g2p_arrivals<DIM, 1, false>), g, dim3(256), 0, s, dev, side, epoch); break;
        case G2pVariant::neo_hookean_plastic: hipLaunchKernelGGL((k_g2p_arrivals<DIM, 1, true>), g, dim3(256), 0, s, dev, side, epoch); break;
        default: hipLaunchKernelGGL((k_g2p_arrivals<DIM, 2, false>), g, dim3(256), 0, s, dev, side, epoch); break;
    }
}

// ---- the launch plans: which shape a substep's launches take (what begin_substep decided is in d->sub and d->dev)

enum class SortBin { full, rebin, by_last_g2p };   // launch 1: k_bin | k_rebin | it ran inside the previous substep's fused G2P
struct SortLaunch {
    bool refresh, reset_table;   // k_table_refresh in front of the sort | reset_hmap, amortised (device_math.h)
    SortBin bin;
    uint32_t do_bodies;          // a pending integrate_bodies of the previous substep rides in workgroup 0 of launch 1
    uint32_t nscan, nreg;        // launch 2: scan and regroup workgroups; have_old, cdf, summ: launch_regroup
    int have_old;
    bool cdf, summ;
    uint32_t refresh_wgs, mesh_wgs, p2g_cdf_wgs;   // k_table_refresh; k_rigid_transform / _mark / _touch; k_p2g_cdf
};
SortLaunch plan_sort(const wgs_data *d) {
    const Dev &dev = d->dev;
    SortLaunch p{};
    // the marks of evicted blocks crowd the table (the host's last look): clear it and insert the live blocks again under
    // their own ids — no particle is touched, the steady-state sort goes on (kernels_sort.h k_table_refresh)
    p.refresh = d->seen.force_refresh && !d->sub.rehash && dev.free_ids != nullptr;
    p.refresh_wgs = std::max(1u, std::min((dev.cap + 255u) / 256u, (uint32_t)grid_for(d, 4)));
    p.reset_table = d->sub.rehash;
    // (sharded runs: k_rebin also bins the particles that arrived in the last substep, behind the residents)
    p.bin = d->sub.binned ? SortBin::by_last_g2p : d->sub.use_rebin ? SortBin::rebin : SortBin::full;
    p.do_bodies = d->sub.bodies_pending ? 1u : 0u;
    p.mesh_wgs = (uint32_t)grid_for(d, 1);
    p.nscan = (dev.cap + SCAN_CHUNK - 1) / SCAN_CHUNK;
    // one resident round: 4 workgroups per CU (127 VGPRs, 36 KB of LDS), the scan workgroups among them
    p.nreg = std::max(1u, std::min((dev.cap + 3u) / 4u, WGS_REGROUP_ROUNDS * ((uint32_t)grid_for(d, 4) - std::min(p.nscan, (uint32_t)grid_for(d, 2)))));
    p.have_old = d->sub.use_rebin ? 1 : 0;
    p.cdf = d->sub.fused_cdf;
    // (summ: every block within reach of a collider is evaluated substep after substep — each evaluates its own nodes and
    // tells its neighbours, kernels_sort.h block_cdf_summ; with colliders at rest: the instantiation without)
    p.summ = (dev.cdf_moving != 0u || dev.cdf_gen == 0u) && !(dev.dbg & DBG_NO_CDF_SUMM);
    p.p2g_cdf_wgs = std::min((dev.n_rigid * 32u + 255u) / 256u, (uint32_t)grid_for(d, 32));
    return p;
}

// which blocks a P2G launch takes (kernels_transfer.h layer_sel): all of them, or — the split form of a slab's phase A,
// host_sharded.inc — the boundary layers with the pack waves behind them, then all other blocks with the interior's grid update
enum class P2gLayers { all, boundary, others };

// The shape of this substep's P2G.
P2gLaunch plan_p2g(const wgs_data *d, P2gLayers layers) {
    const Dev &dev = d->dev;
    const uint32_t n = dev.n;
    const uint32_t NW = (uint32_t)P2GCfg<D>::NW;
    P2gLaunch p{};
    p.two_way = d->two_way;
    p.layer_sel = layers == P2gLayers::boundary ? 1u : layers == P2gLayers::others ? 2u : 0u;
    // Workgroups per body: about one per two entries of the block list (as the host last saw it), between 8 and
    // 32 per CU. A workgroup strides over the list, and the dispatcher balances better than a fixed stride does:
    // blocks differ in cost, and with 5 per CU — one resident round and a quarter — the quarter started when the
    // first workgroups retired (C5, 16 M particles: P2G 472 -> 346 us; C2: 35.6 -> 31.8 us). Same results for
    // any grid: a block's slab is the work of one workgroup.
    p.wgs = std::min((uint32_t)grid_for(d, 32), std::max((uint32_t)grid_for(d, 8), (d->seen.nblocks / 2u + 255u) & ~255u));
    p.gu = d->sub.gu_fused ? 2 : d->sub.shard_fused ? 3 : 0;   // (begin_substep)
    // (8, 16, 32 or 64 workgroups per CU at most: the same times at C2 / C3 / C5)
    const uint32_t gu_wgs = (p.gu == 0 || layers == P2gLayers::boundary) ? 0u : std::min((uint32_t)grid_for(d, 8), std::max((uint32_t)grid_for(d, 1), ((d->seen.nblocks + NW - 1u) / NW + 7u) & ~7u));
    if (d->sub.shard_fused && (d->link->has_lower || d->link->has_upper) && layers != P2gLayers::others) {   // (they ride behind the boundary layers' P2G)
        const PackWaves pw = pack_waves(d);
        p.npack_blk = pw.blocks;
        p.npack = (pw.blocks + pw.guests + NW - 1u) / NW;
    }
    p.ride = p.npack + gu_wgs;
    // Prologue waves (kernels_transfer.h pcdf_waves): the particle cdf of the listed blocks by one wave per visit-list entry in front
    // of the paired launch, while the lists are short enough for the idle part of the chip to take them at once (as of the
    // host's last look: the waves stride over whatever the lists hold now). Single-domain data only: a slab's pack waves read
    // the guests' quads inside the launch.
    if (d->cpic && !dev.sharded && d->seen.nvisit != UINT32_MAX && d->seen.nvisit != 0u && d->seen.nvisit <= PCDF_WAVES_MAX_VISITS && !(dev.dbg & DBG_NO_PCDF_WAVES))
        p.npro = 8u * ((std::min(d->seen.nvisit + 8u, dev.visit_cap) + NW - 1u) / NW);
    if (d->cpic && !dev.sharded && (dev.dbg & DBG_PCDF_WAVES_UNSIZED)) p.npro = 8u;   // (the launch itself then decides, device_math.h pcdf_waves_on)
    if (!d->cpic) {
        p.shape = P2gShape::plain;
        return p;
    }
    // Large one-way collider simulations ALWAYS run the paired launch, with the CPIC body cut to 168 VGPRs: the
    // plain body then keeps its occupancy, so the pair costs nothing while the list is empty, and the choice
    // does not follow the host's syncs (the two budgets differ in the last bit here and there).
    p.small_budget = !d->two_way && n >= P2G_SMALL_BUDGET_MIN_PARTICLES && !(dev.dbg & DBG_NO_P2G_SMALL_BUDGET);
    // Large TWO-WAY simulations never pair: the kernel would take the two-way CPIC body's 225 registers and the plain
    // body — nearly every block — would run at two thirds of its occupancy (C4, 8 M particles: P2G 416 -> 347 us
    // with the two launches). Bit-identical either way (the same body text under -ffp-contract=on).
    const bool big_two_way = d->two_way && n >= P2G_SMALL_BUDGET_MIN_PARTICLES;
    // (small two-way scenes pair whatever the list length: they fill less than one round of workgroups, so the plain body's lost
    // occupancy costs nothing and a launch goes — the reference's sand2, 490 k particles, 2D: 76-79 -> 67-68 us per substep;
    // the one-way 262 k cube: P2G 20.4 + a boundary -> 18.3 us, not taken: its fused G2P then ran 27 us every other run against 21-22)
    const bool small_two_way = d->two_way && n < P2G_SMALL_BUDGET_MIN_PARTICLES;
    // many blocks near colliders (as of the last wgs_sync): both bodies in one launch
    const bool many_listed = d->seen.ncpic != UINT32_MAX && d->seen.ncpic >= P2G_PAIR_MIN_BLOCKS;
    if (!big_two_way && (p.small_budget || small_two_way || many_listed) && !(dev.dbg & DBG_P2G_TWO_LAUNCHES))
        p.shape = P2gShape::pair;
    // Large two-way simulations on a single domain: the near-collider launch FIRST, the plain launch behind it with the grid
    // update riding in IT. The grid-update waves take the registers of the launch they ride in: behind the two-way body (209
    // registers, two waves per SIMD) the update of every block of the scene ran at two thirds of the occupancy it has behind
    // the plain body (160), and started only when the last near-collider workgroup — a 30 us chain each — had a slot. Same
    // sums in the same order (DBG_PLAIN_P2G_FIRST = the plain launch first, as before: tested bit-identical).
    else if (big_two_way && p.gu == 2 && !(dev.dbg & DBG_PLAIN_P2G_FIRST))
        p.shape = P2gShape::cpic_first;
    else
        p.shape = P2gShape::separate;
    return p;
}

// The shape of this substep's fused G2P (dev.g2p_npass set).
G2pLaunch plan_g2p(const wgs_data *d) {
    const Dev &dev = d->dev;
    const uint32_t npass = dev.g2p_npass;
    // the list walk of the CPIC body: a wave and a half per SIMD unless the host saw the visit lists
    const uint32_t full = (uint32_t)grid_for(d, 1) * 3u / 2u;
    G2pLaunch p{G2pShape::single, dev.sharded != 0u, ((dev.nv + G2P_THREADS * npass - 1) / (G2P_THREADS * npass) + 7) / 8 * 8, full};
    // (a slab always takes the paired / single-body launch shapes, the two-launch debug shape exists for single-domain data only)
    if (d->cpic && (p.shard || !(dev.dbg & DBG_G2P_TWO_LAUNCHES))) {
        // both bodies in one launch; list waves (8 x nlist; the waves of an XCD stride over the runs of its visit list): 2 x the
        // runs of the longest list as the host last saw it
        const uint32_t per_run = std::min<uint32_t>(npass, WGS_G2P_LIST_PASSES);
        if (d->seen.nvisit != UINT32_MAX) p.nlist = std::min(full, std::max(8u, 2u * ((d->seen.nvisit + per_run - 1u) / per_run)));
        // plastic scenes with a large share of listed blocks: the spill-free variant (kernels_transfer.h)
        const bool dense = d->plastic && d->seen.ncpic != UINT32_MAX && d->seen.ncpic * 2u >= std::max(1u, d->seen.sync_nblocks) && !(dev.dbg & DBG_NO_G2P_DENSE);
        p.shape = dense ? G2pShape::pair_dense : G2pShape::pair;
    } else if (d->cpic) {
        p.shape = G2pShape::two_launches;
    }
    return p;
}

// ---- the stages. One substep = pipeline.rs:201-280 (MPM passes), enqueued on the data's stream: begin_substep, enqueue_sort,
// enqueue_p2g, enqueue_finish. wgs_step runs them back to back (single-domain data, or a slab stepped without its neighbours);
// the sharded step puts its one neighbour exchange in front of enqueue_finish (host_sharded.inc, also on the split form of P2G).

// The timing marks of the substep being enqueued (Substep::ts_slot; resolve_timings names them) and the developer's trace.
struct Mark {
    wgs_data *d;
    void operator()(int m) const {
        static const bool trace = getenv("WGS_TRACE") != nullptr;   // developer aid: drain the stream at every pass boundary and say so
        if (d->sub.ts_slot >= 0) hipEventRecord(d->timing.events.ev[d->sub.ts_slot][m], d->stream);
        if (trace) {
            const hipError_t te = hipStreamSynchronize(d->stream);
            fprintf(stderr, "[wgs trace] substep %llu mark %d: %s\n", (unsigned long long)d->substeps, m, hipGetErrorString(te));
        }
    }
};

// A slab's counter catch-up: the set of particle counters the coming launches read (layout.h), and the counters of a buffer that
// a substep without neighbours left unset (Substep::needs_compact: only ever set on a slab).
void catch_up_counters(wgs_data *d) {
    d->dev.ctr_set = (uint32_t)(d->substeps & 1u);
    if (!d->sub.needs_compact) return;
    hipLaunchKernelGGL(k_shard_compacted, dim3(1), dim3(64), 0, d->stream, d->dev);
    d->sub.needs_compact = false;
}

// Every decision the launches of one substep share, made once, in front of its first launch: into d->sub what the stages read,
// into d->dev the per-substep kernel arguments. "(same in every stage: ...)" says why a stage that used to compute the value
// itself got this one: no entry point runs between the stages of a substep — a sharded step puts only its exchange and the
// other slabs' stages there (maintain_grid and watch_counters run in front of a substep, fetch_counters in entry points of its own).
wgs_status begin_substep(wgs_data *d, bool in_sharded_step, int ts_slot = -1) {
    Dev &dev = d->dev;
    wgs_data::Substep &sub = d->sub;
    hipStream_t s = d->stream;
    sub.in_sharded_step = in_sharded_step;
    sub.ts_slot = ts_slot;
    sub.epoch = (uint32_t)(d->substeps + 1);   // (same in every stage: `substeps` moves at the end of enqueue_finish only)
    // chunks of 64 sorted particles per wave of the fused G2P (kernels_transfer.h); the sort files the visit list by it
    // (2D: the body keeps no state of the chunk after the next one — at most two chunks per wave)
    // (same in every stage: seen.nv_hint is written by maintain_grid and fetch_counters, dev.nv by enqueue_finish)
    const uint32_t nv_now = dev.sharded && d->seen.nv_hint != 0u ? std::min(d->seen.nv_hint, dev.nv) : dev.nv;   // (a slab launches for its capacity)
    dev.g2p_npass = (D == 3 && nv_now >= G2P_MANY_PASS_MIN_PARTICLES) ? (uint32_t)G2P_MANY_PASSES
                    : (nv_now >= G2P_TWO_PASS_MIN_PARTICLES || (dev.dbg & DBG_G2P_TWO_PASSES)) ? 2u : 1u;
    // Steady state: the buffer is in the sorted order of the previous substep, whose block ids, cell ids
    // (perm_cell) and neighbour links are still valid, so the particles are re-binned RELATIVE to their old
    // block (k_rebin: no hash lookups except for the few particles that changed block). The full k_bin runs
    // on the first substep, on table-rebuild substeps and in sharded runs (particles arrive from neighbours).
    // (read by the sort only: a later stage used to compute it again without the consumed force_rehash, for nobody)
    sub.rehash = d->substeps == 0 || (d->rehash_period != 0u && d->substeps % d->rehash_period == 0) || d->seen.force_rehash;
    if (sub.rehash) {
        d->stats.table_rebuilds++;
        d->seen.force_rehash = false;
        d->cdf_generation++;   // block ids are handed out anew
    }
    // node cdfs / block classes are reused from one substep to the next while no collider can move
    // (same in every stage: cdf_generation and moving_mask move here and in setters, which are entry points)
    dev.cdf_gen = d->cpic ? d->cdf_generation : 0u;
    dev.cdf_moving = d->moving_mask;
    sub.fused_cdf = d->cpic && dev.n_rigid == 0;  // (mesh cdfs are only complete after k_p2g_cdf)
    dev.listed_in_perm = sub.fused_cdf ? 1u : 0u;  // (written once per substep as before: enqueue_finish consumes what the sort wrote)
    sub.use_rebin = sub.prev_sorted && !sub.rehash && !(dev.dbg & DBG_NO_REBIN);   // (read by the sort only, like `binned`)
    // The fused G2P of this substep also bins its output for the next one (g2p_body.inc, Dev::bin_next; slabs too), unless
    // that substep rebuilds the table anyway (DBG_REBIN_LAUNCH brings launch 1 of the sort, k_rebin, back: same results, tested).
    // `prebinned`: the previous substep's G2P did so for this one.
    sub.binned = sub.use_rebin && sub.prebinned;
    if (sub.prebinned && !sub.binned) {
        // (a table rebuild nobody could foresee — ids three quarters handed out, seen by the host in between: what the G2P
        // accumulated for the old ids is dropped; the stamps it left mean nothing once the ids are handed out anew)
        HIP_TRY(hipMemsetAsync(dev.block_acc, 0, sizeof(uint32_t) * (size_t)dev.cap, s));
        HIP_TRY(hipMemsetAsync(dev.cell_head, 0, sizeof(uint32_t) * (size_t)dev.cap * NPB, s));
        HIP_TRY(hipMemsetAsync(dev.blk_narr, 0, sizeof(uint32_t) * (size_t)dev.cap, s));
    }
    sub.prebinned = false;
    // (not the plastic variants: their fused G2P is compiled without the binning — kernels_transfer.h: the code alone, beyond the
    // instruction cache, cost a third of the launch — and launch 1 of the sort, k_rebin, stays)
    // (a slab: its fused G2P bins the residents — the guests it drops leave their block's total —, k_g2p_arrivals the particles that
    // arrive. Same in every stage: the data's plasticity, switches and rebuild period are fixed, `substeps` as for the epoch)
    dev.bin_next = (!d->plastic && !(dev.dbg & (DBG_NO_REBIN | DBG_REBIN_LAUNCH)) && (d->rehash_period == 0u || (d->substeps + 1) % d->rehash_period != 0)) ? 1u : 0u;
    // the fused G2P drops the guests only inside the sharded step (kernels_shard.h); wgs_step on a slab advances what it holds
    dev.skip_guests = (in_sharded_step && dev.sharded) ? 1u : 0u;
    // Single-domain simulations: the grid update rides in the (last) P2G launch as workgroups of its own
    // behind the P2G workgroups (kernels_transfer.h gu_waves; GU = 2), one wave per active block as the host last saw
    // them; a P2G launch before it hands its slabs over the same way (GU = 1). Same results as the launch of its own
    // (DBG_GU_OWN_LAUNCH): the same sums in the same order.
    sub.gu_fused = !in_sharded_step && !dev.sharded && !(dev.dbg & DBG_GU_OWN_LAUNCH);
    // Inside wgs_sharded_step: behind the P2G workgroups ride the waves that pack the outgoing messages (no k_pack_face launch)
    // and the grid update of the INTERIOR blocks — everything that does not wait for the exchange; the interface layers are updated
    // after it (GU = 3). (an empty slab launches no P2G for them to ride in. Same in every stage: attaching a slab is an entry point)
    const bool attached = in_sharded_step && d->link && d->link->attached;
    sub.shard_fused = attached && dev.n > 0 && !(dev.dbg & DBG_GU_OWN_LAUNCH);
    sub.arrivals = attached;
    catch_up_counters(d);   // (a slab last stepped by wgs_step: k_shard_compacted at the head of this substep)
    return WGS_OK;
}

// marks 0..3 — "grid sort" (grid.rs:30-207), then the node and particle cdfs of mesh colliders
template <int DIM> wgs_status enqueue_sort(wgs_data *d) {
    Dev &dev = d->dev;
    hipStream_t s = d->stream;
    const Mark mark{d};
    const int side = d->side;
    const uint32_t n = dev.n, epoch = d->sub.epoch;
    const int pgrid = (int)((n + SORT_THREADS - 1) / SORT_THREADS);
    const SortLaunch p = plan_sort(d);
    if (d->sub.ts_slot >= 0) {  // two adjacent marks: their distance is what every interval below pays for its closing mark
        mark(9);
        mark(10);
    }
    mark(0);
    if (p.refresh) {
        WGS_TRY(clear_table(d, false));
        hipLaunchKernelGGL(k_table_refresh, dim3(p.refresh_wgs), dim3(256), 0, s, dev);
        d->stats.table_refreshes++;
    }
    d->seen.force_refresh = false;
    if (p.reset_table) WGS_TRY(clear_table(d, true));
    // ---- "update rigid particles" (rigid_particle_update.wgsl): samples and vertices of the mesh colliders
    if (dev.n_rigid > 0)
        hipLaunchKernelGGL(k_rigid_transform<DIM>, dim3(p.mesh_wgs), dim3(256), 0, s, dev);
    if (n > 0) {
        d->sub.bodies_pending = false;   // (p.do_bodies)
        switch (p.bin) {
            case SortBin::by_last_g2p: if (p.do_bodies) launch_bodies_integrate(d); break;
            case SortBin::rebin: hipLaunchKernelGGL(k_rebin<DIM>, dim3((pgrid + REBIN_K - 1) / REBIN_K), dim3(SORT_THREADS), 0, s, dev, side, epoch, p.do_bodies); break;
            case SortBin::full: hipLaunchKernelGGL(k_bin<DIM>, dim3(pgrid), dim3(SORT_THREADS), 0, s, dev, side, epoch, p.do_bodies); break;
        }
        if (dev.n_rigid > 0) {  // blocks a mesh sample reaches must exist (sort.wgsl:38-86)
            hipLaunchKernelGGL(k_rigid_mark<DIM>, dim3(p.mesh_wgs), dim3(256), 0, s, dev, epoch);
            hipLaunchKernelGGL(k_rigid_touch<DIM>, dim3(p.mesh_wgs), dim3(256), 0, s, dev, epoch);
        }
        // launch 2: chunked scan (active list, first_particle) + per-block setup and regrouping in canonical order.
        // Collider simulations without mesh colliders: node cdf + block classes ride in this launch, the particle
        // cdf in the CPIC P2G launch (no CDF launch at all)
        launch_regroup<DIM>(dev, s, dim3(p.nscan + p.nreg), side, epoch, p.nscan, p.have_old, p.cdf, p.summ);
    } else {
        HIP_TRY(hipMemsetAsync(dev.counters + CTR_NBLOCKS, 0, sizeof(uint32_t), s));
    }
    mark(1);
    // ---- "grid_update_cdf" + "g2p_cdf" (collide.wgsl, grid_update_cdf.wgsl, g2p_cdf.wgsl): one launch
    // (kernels_cdf.h); the reference's two pass names share its time in wgs_read_timings
    if (dev.n_rigid > 0 && n > 0)  // "p2g_cdf": mesh primitives -> node cdf accumulators
        hipLaunchKernelGGL(k_p2g_cdf<DIM>, dim3(p.p2g_cdf_wgs), dim3(256), 0, s, dev, epoch);
    if (d->cpic && n > 0 && !p.cdf)
        hipLaunchKernelGGL(k_cdf<DIM>, dim3(grid_for(d, 16)), dim3(CDF_THREADS), 0, s, dev, side, epoch);
    mark(2);
    mark(3);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

// mark 4 — "p2g", with what rides behind its workgroups (plan_p2g)
template <int DIM> wgs_status enqueue_p2g(wgs_data *d, P2gLayers layers) {
    if (d->dev.n > 0) launch_p2g<DIM>(d->dev, d->stream, d->side, d->sub.epoch, plan_p2g(d, layers));
    Mark{d}(4);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

// marks 5..8 — grid update, fused G2P, a slab's arrivals, bodies; then the substep is over
template <int DIM> wgs_status enqueue_finish(wgs_data *d) {
    Dev &dev = d->dev;
    const wgs_data::Substep &sub = d->sub;
    hipStream_t s = d->stream;
    const Mark mark{d};
    const int side = d->side;
    const uint32_t n = dev.n, epoch = sub.epoch;
    // ---- "grid_update" (single-domain simulations: done by waves of the P2G launch above)
    if (n > 0 && !sub.gu_fused)
        launch_grid_update<DIM>(dev, s, dim3(grid_for(d, WGS_GU_WG_PER_CU)), epoch, sub.in_sharded_step, d->two_way, sub.shard_fused ? 1u : 0u);
    // ---- force fields (wgs_set_force_fields; no reference counterpart): behind either form of the grid update and in front of the
    // walls, whose postconditions keep holding; a launch of its own — data without fields launches what it always did
    if (n > 0 && d->forces_set) launch_grid_forces(d);
    // ---- domain walls (wgs_set_domain_walls; no reference counterpart): the wall nodes' velocities are projected behind either
    // form of the grid update, in nodes and slabs alike, in a launch of its own — data without walls launches what it always did
    if (n > 0 && d->walls_set) launch_grid_walls(d);
    mark(5);
    // ---- "g2p" + "particles_update", fused (mark 6: between the two launches of a collider simulation's G2P)
    const G2pLaunch g2p = plan_g2p(d);
    if (dev.nv > 0) launch_g2p<DIM>(dev, s, side, epoch, d->plastic, d->plasticity, g2p, mark);
    if (!(dev.nv > 0 && g2p.shape == G2pShape::two_launches)) mark(6);
    // sharded step: the particles that arrived with this substep's messages are advanced too (kernels_arrivals.h), by a
    // launch of their own behind the fused G2P. (As extra workgroups INSIDE that launch — first or last in its grid — they
    // made it 7-10 us longer at a 1 M slab for the 5 us launch they saved: measured twice in round 3, not kept.)
    // (the arrivals' body also does the bookkeeping of the migration round, so it runs even when nobody can arrive)
    if (sub.arrivals) {
        const uint32_t arr_most = ((d->link->has_lower ? 1u : 0u) + (d->link->has_upper ? 1u : 0u)) * d->link->mig_cap;
        launch_arrivals<DIM>(dev, s, dim3(std::max(1u, std::min((arr_most + ARR_PER_WG - 1u) / ARR_PER_WG, 1024u))), side, epoch, d->plastic);
    }
    mark(7);
    // ---- "integrate_bodies" (rigid_impulses.wgsl:95-136) + the world mass properties of the next substep
    // (pipeline.rs:204-205). Skipped while no body has a velocity or a mass: it would be the identity.
    // (reduce_impulses is read HERE, not in begin_substep: the lockstep step sets it between a slab's two phases; 2 = the group sums and integrates)
    if (d->bodies_move && dev.n_colliders > 0 && !(sub.in_sharded_step && d->reduce_impulses == 2)) {
        if (sub.in_sharded_step && d->reduce_impulses == 1) WGS_TRY(allreduce_impulses(d));
        // Single-domain simulations without mesh colliders: left to the first launch of the next substep (or to the end of
        // this wgs_step call, flush_bodies) — a 16-thread launch of its own costs a dependent launch, ~5 us, per substep.
        // (not when this substep's G2P binned for the next one: that substep has no launch in front of the node cdfs of its sort)
        if (!sub.in_sharded_step && !dev.sharded && dev.n_rigid == 0 && n > 0 && !(dev.dbg & DBG_BODIES_OWN_LAUNCH) && !dev.bin_next) d->sub.bodies_pending = true;
        else launch_bodies_integrate(d);
    }
    mark(8);
    d->side ^= 1;
    d->substeps++;
    d->sub.prev_sorted = true;
    d->sub.prebinned = dev.bin_next != 0u && dev.nv > 0;
    dev.n = dev.nv;  // the buffer just written holds the valid particles only, in sorted order
    // sharded: the counters of the new buffer (CTR_N / CTR_NPREV / CTR_NV) are set by k_g2p_arrivals; a slab stepped
    // without its neighbours (wgs_step) sets them at the head of its next substep (k_shard_compacted)
    if (dev.sharded && !sub.arrivals) d->sub.needs_compact = true;
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

// integrate_bodies in a launch of its own: where no sort launch carries it
void launch_bodies_integrate(wgs_data *d) { hipLaunchKernelGGL(k_bodies_integrate<D>, dim3(1), dim3(16), 0, d->stream, d->dev); }

// integrate_bodies of a lockstep group (the group summed the impulses of its slabs after every slab's grid update)
wgs_status enqueue_bodies(wgs_data *d) {
    if (d->bodies_move && d->dev.n_colliders > 0) launch_bodies_integrate(d);
    HIP_TRY(hipGetLastError());
    return WGS_OK;
}

}  // namespace
