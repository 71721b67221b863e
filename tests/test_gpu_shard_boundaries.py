"""The slab exchange (kernels_shard.h pack_face_body / rec_claim / rec_find, arrivals_body.inc, the leavers' list) at every capacity and
wave boundary, at the boundary's exact value and one to either side: one case per row of shard_truth.ROWS, as a lockstep group on one GPU
(wgs_sharded_step_lockstep), and `mig-65` once more through wgs_sharded_step over RCCL with the rank as its own neighbours.

A passing row steps K - 2 substeps and exports `pos_a`, one more and exports `pos_b`, then the checked substep K, whose messages carry the
leavers of substep K - 1. From what the slabs themselves export:
  * shard_truth.check_facts: leavers, held particles and halo records equal the row's designed counts, with ==; every slab holds exactly
    the ids the truth names, before and after the checked substep, and stats()["num_particles"] says the same number;
  * join_slabs(...).exact: no id lost, none held twice; sync() clean on every slab, overflow == 0;
  * the same case with generous capacities gives the same bits slab by slab (by_id over ids, pos, vel, def_grad, affine): a capacity never
    changes a result — also under GU_OWN_LAUNCH, SHARD_SPLIT_LAYERS and REBIN_LAUNCH on the mig-both, halo-at and halo-steady-and-new rows;
  * the joined state is within gpu_common.PART_TOL (relative RMS, pos and vel) of the single-domain GPU run of the same scene.
An over-capacity row steps up to and including the substep of the overflow and no further; sync() then raises on the slabs the row names,
with the message of ERRBIT_SHARD, and is clean on the others; the handles are destroyed, nothing is asserted about their particles. These
are the reported error paths of the exchange, each bounds-guarded (a slot that is not granted is not written)."""
import numpy as np
import pytest

from wgsparkl_amd._ffi import WgsError
from wgsparkl_amd.selfcheck import rel_rms
from wgsparkl_amd.sharded import NativeComm, NativeShard, SlabPartition, by_id, join_slabs, native_lockstep, split_scene, uniform_material_of

from helpers import debug, pipeline, report_margin, run_gpu
from gpu_common import PART_TOL
import shard_truth as T
from shard_truth import GENEROUS, MIN_INTERIOR_WIDTH, ROW

pytestmark = pytest.mark.gpu

OVERFLOWED = "a message buffer or the particle capacity overflowed"
FIELDS = ("ids", "pos", "vel", "def_grad", "affine")
PASSING = [r.name for r in T.ROWS if r.over is None]
OVER = [r.name for r in T.ROWS if r.over is not None]
SWITCHED = [n for n in PASSING if n.startswith(("mig-both", "halo-at", "halo-steady-and-new"))]


def _slabs(row, sc, generous=False):
    """the row's lockstep group: per-slab particle capacities, the row's message capacities (`generous`: GENEROUS records and migrants — twice
    the row's where it asks for more than that —, room for every particle of the scene)"""
    ps, part = sc["particles"], T.part_of(row)
    halo_cap, mig_cap, capacity = T.capacities(row, sc)
    if generous:
        halo_cap, mig_cap = max(GENEROUS, 2 * halo_cap), max(GENEROUS, 2 * mig_cap)
        capacity = [max(c, ps.n) for c in capacity]
    pipe = pipeline(row.dim)
    slab = {**sc, "partition": part, "uniform_material": uniform_material_of(ps)}
    shards = [NativeShard.from_scene(pipe, {**slab, "particles": sub, "global_ids": gids}, r, particle_capacity=capacity[r],
                                     halo_capacity_records=halo_cap, migrant_capacity=mig_cap)
              for r, (sub, gids) in enumerate(split_scene(ps, part, sc["cell_width"]))]
    return pipe, shards


def _close(shards):
    for s in shards:
        s.close()


def _snapshot(shards, n):
    for s in shards:
        s.sync()
    outs = [s.export() for s in shards]
    joined = join_slabs(outs, np.arange(n))
    assert joined.exact, joined.problem
    for s, o in zip(shards, outs):
        st = s.stats()
        assert st["num_particles"] == len(o["ids"]) and st["overflow"] == 0, st
    return joined, outs


def _run(row, sc, generous=False, checked=True):
    """the row's case; returns (the slabs' exports by id, the joined state) after the checked substep"""
    pipe, shards = _slabs(row, sc, generous)
    try:
        n, k = sc["particles"].n, row.substeps
        pos_a = None
        if k >= 2:
            if k > 2:
                native_lockstep(pipe, shards, k - 2)
            pos_a = _snapshot(shards, n)[0].fields["pos"]
            native_lockstep(pipe, shards, 1)
        joined_b, outs_b = _snapshot(shards, n)
        pos_b = joined_b.fields["pos"]
        if checked:
            T.check_facts(row, pos_a, pos_b, held_ids=[o["ids"] for o in outs_b])
        native_lockstep(pipe, shards, 1)
        joined_c, outs_c = _snapshot(shards, n)
        if checked:        # after the exchange: the migrants are their new owner's, once
            T.check_facts(row._replace(leavers=None, held=None, halo=None), pos_b, joined_c.fields["pos"], held_ids=[o["ids"] for o in outs_c])
        return [by_id(o) for o in outs_c], joined_c
    finally:
        _close(shards)


def _same_bits(a, b, what):
    for r, (x, y) in enumerate(zip(a, b)):
        for f in FIELDS:
            assert x[f].tobytes() == y[f].tobytes(), (what, r, f)


@pytest.mark.parametrize("name", PASSING)
def test_boundary_case(hip_libs, monkeypatch, name):
    row = ROW[name]
    sc = T.build(row)
    outs, joined = _run(row, sc)
    twin, _ = _run(row, sc, generous=True, checked=False)
    _same_bits(outs, twin, "generous capacities")
    if name in SWITCHED:
        for switch in ("GU_OWN_LAUNCH", "SHARD_SPLIT_LAYERS", "REBIN_LAUNCH"):
            with debug(monkeypatch, switch):
                other, _ = _run(row, sc, checked=False)
            _same_bits(outs, other, switch)
    ref = run_gpu(sc, row.substeps).read_particles()
    for f in ("pos", "vel"):
        err = rel_rms(joined.fields[f], getattr(ref, f))
        print(f"{name}: {f} rel rms vs the single-domain run {err:.3e} (bound {PART_TOL:.0e})")
        report_margin(f"slab boundaries {f} vs single domain", err, PART_TOL)
        assert err < PART_TOL, (f, err)
    if row.exact:
        flip = T.flip_x(row.dim)
        x = joined.fields["pos"][:, 0]
        for v in (np.nextafter(flip, np.float32(-np.inf)), flip, np.nextafter(flip, np.float32(np.inf))):
            assert (x == v).sum() == 2, "the particles on the cut moved"


@pytest.mark.parametrize("name", OVER)
def test_over_capacity_is_reported(hip_libs, name):
    row = ROW[name]
    sc = T.build(row)
    substep, reporters = row.over
    pipe, shards = _slabs(row, sc)
    try:
        native_lockstep(pipe, shards, substep)        # up to and including the substep of the overflow, not one further
        for r, s in enumerate(shards):
            if r in reporters:
                with pytest.raises(WgsError) as e:
                    s.sync()
                assert OVERFLOWED in str(e.value), (r, str(e.value))
            else:
                s.sync()
    finally:
        _close(shards)


def test_the_substep_before_an_overflow_is_clean(hip_libs):
    """the over rows report in the substep the row names and not earlier: one substep less, and every slab syncs clean"""
    for name in ("migcap-over-64-3d", "room-over-2-guests-2d", "leavers-%d-3d" % (T.LEAVERS_MIN + 1)):
        row = ROW[name]
        pipe, shards = _slabs(row, T.build(row))
        try:
            native_lockstep(pipe, shards, row.over[0] - 1)
            for s in shards:
                s.sync()
        finally:
            _close(shards)


def test_attach_refuses_a_zero_capacity_and_a_narrow_middle_slab(hip_libs):
    row = ROW["mig-both-1+1-3d"]
    sc = T.build(row)
    ps, pipe = sc["particles"], pipeline(3)
    b = T.first_cut(3)
    part = SlabPartition([b - 64, b, b + MIN_INTERIOR_WIDTH - 1, b + 64])
    slab = {**sc, "partition": part, "uniform_material": uniform_material_of(ps)}
    sub, gids = split_scene(ps, part, sc["cell_width"])[1]
    with pytest.raises(WgsError, match="a slab with two neighbours must be at least 3 blocks wide"):
        NativeShard.from_scene(pipe, {**slab, "particles": sub, "global_ids": gids}, 1, particle_capacity=ps.n)
    slab["partition"] = T.part_of(row)
    sub, gids = split_scene(ps, slab["partition"], sc["cell_width"])[1]
    for kw in (dict(halo_capacity_records=0), dict(migrant_capacity=0)):
        with pytest.raises(WgsError, match="zero message capacity"):
            NativeShard.from_scene(pipe, {**slab, "particles": sub, "global_ids": gids}, 1, particle_capacity=ps.n, **kw)
    NativeShard.from_scene(pipe, {**slab, "particles": sub, "global_ids": gids}, 1, particle_capacity=ps.n).close()    # (the same call, wide enough)


def test_mig_65_over_rccl_as_its_own_neighbours(hip_libs):
    """Slab 0 of mig-65-3d through wgs_sharded_step with WGS_COMM_SELF_NEIGHBOURS: every send is matched by the rank's own receive, so the 65
    leavers of substep K - 1 travel in the upper message of substep K (migrant_capacity 65: exactly full) and come back as arrivals —
    which the arrivals' kernel finds outside the core range and lists again. The nodes the slab shares with itself hold twice the
    momentum and twice the mass: the same velocity, so the cloud still translates rigidly. Nobody is lost, nothing is reported."""
    row = ROW["mig-65-3d"]
    sc = T.build(row)
    ps, part = sc["particles"], T.part_of(row)
    pipe = pipeline(3)
    sub, gids = split_scene(ps, part, sc["cell_width"])[0]
    assert sub.n == 6 + 65
    comm = NativeComm(pipe, None, 0, 1, flags=1)
    sh = NativeShard(pipe, sc["params"], sub, gids, sc["colliders"], sc["cell_width"], sc["grid_capacity"], part.cuts[0], part.cuts[1], True, True,
                     2 * sub.n, sc["model"], comm=comm, halo_capacity_records=64, migrant_capacity=65, uniform_material=uniform_material_of(ps))
    try:
        pos = {}
        for k in range(row.substeps - 2, row.substeps + 2):
            sh.step(k if not pos else 1)
            sh.sync()
            out = by_id(sh.export())
            assert np.array_equal(out["ids"], np.sort(gids)), f"after substep {k}: the slab holds {len(out['ids'])} of its {sub.n} particles"
            assert sh.stats()["num_particles"] == sub.n and sh.stats()["overflow"] == 0
            pos[k] = out["pos"]
            want = T.designed(sc, k)[np.sort(gids)]
            assert np.abs(pos[k] - want).max() < 2e-4, (k, np.abs(pos[k] - want).max())
        outside = lambda p: int((T.owner(p, part, 3) != 0).sum())
        assert [outside(pos[k]) for k in sorted(pos)] == [0, 65, 65, 65]
    finally:
        sh.close()
        comm.close()
