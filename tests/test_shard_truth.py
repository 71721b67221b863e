"""CPU twins of tests/test_gpu_shard_boundaries.py: every row of shard_truth.ROWS stepped on tests/shard_oracle.OracleShard — the exchange
protocol restated on the C oracle, fp64 (the on-the-cut rows fp32: their point is the float32 on the cut) — translates rigidly and meets
exactly the leavers, held particles and halo records it was designed for, and the oracle's own messages hold as many records and migrants
as shard_truth says; the table covers every threshold at its value and to either side and is exactly the required cases; the parsed
constants are the sources'; and the checks the GPU file applies reject a halo rule without the regular pair, a leaver attributed to the
wrong face and a slab that is said not to hold the last substep's leavers."""
import collections

import numpy as np
import pytest

from wgsparkl_amd import sharded
from wgsparkl_amd.sharded import join_slabs, split_scene

import shard_truth as T
from shard_oracle import OracleShard
from shard_truth import ARR_MAX_WGS, ARR_PER_WG, GENEROUS, LEAVERS_DIV, LEAVERS_MIN, MIN_INTERIOR_WIDTH, ROW, ROWS, WAVE

_BIG = {}        # the rows of thousands of particles are stepped once per module


def oracle_run(row):
    """The row's scene on OracleShards in lockstep, substep by substep. Returns (pos, held, msgs): pos[k] the positions of all particles by
    id after k substeps (float32), held[k] the ids per slab then, msgs[k] = {(slab, face): (halo records, migrants)} of substep k's messages."""
    if row.name in _BIG:
        return _BIG[row.name]
    sc = T.build(row)
    ps, part = sc["particles"], T.part_of(row)
    dtype = np.float32 if row.exact else np.float64
    shards = []
    for r, (sub, gids) in enumerate(split_scene(ps, part, sc["cell_width"])):
        lo, hi = part.block_range(r)
        shards.append(OracleShard(sc, sub, gids, lo, hi, r > 0, r < part.world - 1, dtype=dtype))

    def snapshot():
        joined = join_slabs([s.export() for s in shards], np.arange(ps.n), fields=("pos",))
        assert joined.exact, joined.problem
        return joined.fields["pos"].astype(np.float32), [np.sort(s.gids) for s in shards]
    pos, held, msgs = [None] * (row.substeps + 1), [None] * (row.substeps + 1), [None] * (row.substeps + 1)
    pos[0], held[0] = snapshot()
    for k in range(1, row.substeps + 1):
        out = [s.begin() for s in shards]
        msgs[k] = {(r, f): (int(m[0]), int(m[1])) for r, pair in enumerate(out) for f, m in enumerate(pair) if m is not None and (m[0] or m[1])}
        for r, s in enumerate(shards):
            s.end(out[r - 1][1] if r > 0 else None, out[r + 1][0] if r < len(shards) - 1 else None)
        pos[k], held[k] = snapshot()
    if ps.n > 2000:
        _BIG[row.name] = (pos, held, msgs)
    return pos, held, msgs


@pytest.mark.parametrize("name", list(ROW))
def test_row_meets_its_designed_counts_on_the_oracle(oracle_libs, name):
    row = ROW[name]
    sc = T.build(row)
    k, part = row.substeps, T.part_of(row)
    assert sc["particles"].dim == row.dim and sc["particles"].n <= 8600
    if not row.exact:
        for j in range(k + 1):
            assert T.off_faces(T.designed(sc, j)).min() >= 0.02, "a particle comes closer than 0.02 cells to a cell face"
    pos, held, msgs = oracle_run(row)
    for j in range(k + 1):       # the cloud translates rigidly: each group at its own velocity
        assert np.abs(pos[j] - T.designed(sc, j)).max() < 2e-4, (j, np.abs(pos[j] - T.designed(sc, j)).max())
    pos_a = pos[k - 2] if k >= 2 else None
    fx = T.check_facts(row, pos_a, pos[k - 1], held_ids=held[k - 1])
    # the oracle's own messages of the checked substep: as many halo records and migrants as the truth says
    lv, _, halo = T.counts(fx)
    keys = set(lv) | set(halo)
    assert {key: (halo.get(key, 0), lv.get(key, 0)) for key in keys} == msgs[k], (halo, lv, msgs[k])
    # and after it: every particle held once, by the slab the truth names
    T.check_facts(row._replace(leavers=None, held=None, halo=None), pos[k - 1], pos[k], held_ids=held[k])
    if row.name.startswith("halo-steady-and-new"):
        assert [m.get((1, 0), (0, 0))[0] for m in msgs[1:]] == T.GROWING_LOWER[row.dim]
        assert [n.get((1, 0), 0) for n in T.needs_over_time(row, sc)] == T.GROWING_LOWER[row.dim]
    if row.exact:
        flip = T.flip_x(row.dim)
        x0 = sc["particles"].pos[:, 0]
        for x in (np.nextafter(flip, np.float32(-np.inf)), flip, np.nextafter(flip, np.float32(np.inf))):
            assert (x0 == x).sum() == 2
        own = T.owner(pos[0], part, row.dim)
        assert (own[x0 <= flip] == 0).all() and (own[x0 > flip] == 1).all(), "the cut is not where flip_x says"
        if row.build[1]["mover"]:
            assert (pos[1][:, 0] == flip).sum() == 3, "the mover does not land exactly on the cut"


# ------------------------------------------------------------------------------------------------ coverage
def _relation(delta):
    return "free" if delta is None or delta > 0 else ("at" if delta == 0 else "over")


def _signature(row):
    """what a row drives, from its designed positions and capacities alone (not from its name, family or expectations)"""
    sc = T.build(row)
    part, k = T.part_of(row), row.substeps
    halo_cap, mig_cap, capacity = T.capacities(row, sc)
    fx = T.facts(part, row.dim, T.designed(sc, k - 2) if k >= 2 else None, T.designed(sc, k - 1))
    lv, held, _ = T.counts(fx)
    needs = T.needs_over_time(row, sc)
    most = max(max(n.values()) for n in needs)
    arrivals = [sum(n for (r, f), n in lv.items() if r + (1 if f else -1) == dst) for dst in range(part.world)]
    guests = [sum(n for (r, f), n in lv.items() if r == src) for src in range(part.world)]
    sig = [row.dim, part.world, tuple(sorted(lv.items()))]
    sig.append(("mig", _relation(mig_cap - max(lv.values(), default=0) if mig_cap != GENEROUS else None)))
    sig.append(("halo", _relation(halo_cap - most if halo_cap != GENEROUS else None), most if halo_cap != GENEROUS and halo_cap - most <= 0 else None))
    room = [c - h - a for c, h, a in zip(capacity, held, arrivals)] if row.capacity is not None and min(capacity) < sc["particles"].n else None
    sig.append(("room", _relation(min(room) if room else None), guests[int(np.argmin(room))] if room else None))
    lcap = [T.leavers_cap(c) for c in capacity]
    sig.append(("leavers", [g - c for g, c in zip(guests, lcap) if g - c >= -1] or None))
    per_trip = [min(-(-(int(part.block_range(r)[0] > sharded.INT_MIN) + int(part.block_range(r)[1] < sharded.INT_MAX)) * mig_cap // ARR_PER_WG), ARR_MAX_WGS)
                * ARR_PER_WG for r in range(part.world)]
    taken = [sum(min(n, mig_cap) for (r, f), n in lv.items() if r + (1 if f else -1) == dst) for dst in range(part.world)]      # n_in = min(header count, mig_cap)
    sig.append(("trips", max(-(-a // p) for a, p in zip(taken, per_trip))))
    if row.exact:
        flip = T.flip_x(row.dim)
        x0, x1 = sc["particles"].pos[:, 0], T.designed(sc, 1)[:, 0]
        sig.append(("cut", tuple(int((x0 == x).sum()) for x in (np.nextafter(flip, np.float32(-np.inf)), flip, np.nextafter(flip, np.float32(np.inf)))),
                    int((x1 == flip).sum() - (x0 == flip).sum())))
    if len({tuple(sorted(n.items())) for n in needs}) > 1 and not lv and not row.exact:
        sig.append(("lower message", tuple(n.get((1, 0), 0) for n in needs)))
    return tuple(str(s) for s in sig)


def _required():
    req = []

    def case(dim, world, lv, mig="free", halo=("free", None), room=("free", None), leavers=None, trips=1, *more):
        return tuple(str(s) for s in (dim, world, tuple(sorted(lv.items())), ("mig", mig), ("halo",) + halo, ("room",) + room, ("leavers", leavers), ("trips", trips)) + more)
    for d in (3, 2):
        both = 4 if d == 3 else 2
        for n in (0, 1, ARR_PER_WG - 1, ARR_PER_WG, ARR_PER_WG + 1, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE, 2 * WAVE + 1):
            req.append(case(d, 2, {(0, 1): n} if n else {}, trips=1 if n else 0))
        for n in (1, WAVE, WAVE + 1):
            req.append(case(d, 2, {(0, 1): n}, mig="at"))
            req.append(case(d, 2, {(0, 1): n + 1 if n == 1 else n}, mig="over"))
        for a, b in ((1, 1), (5, 3), (31, 33), (64, 64)):
            req.append(case(d, 3, {(1, 0): a, (1, 1): b, (0, 1): a, (2, 0): b}, mig="at"))
        for g in (0, 2):
            lv = {(0, 1): 5, (1, 0): g} if g else {(0, 1): 5}
            req += [case(d, 2, lv, room=("at", g)), case(d, 2, lv, room=("over", g))]
        req.append(case(d, 2, {}, "free", ("free", None), ("free", None), None, 0, ("cut", (2, 2, 2), 0)))
        req.append(case(d, 2, {}, "free", ("free", None), ("free", None), None, 0, ("cut", (2, 2, 2), 1)))
        for need in (both, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 2):
            req += [case(d, 2, {}, halo=("at", need), trips=0), case(d, 2, {}, halo=("over", need), trips=0)]
        req.append(case(d, 2, {}, "free", ("at", 4 * both + 1), ("free", None), None, 0, ("lower message", tuple(T.GROWING_LOWER[d]))))
    for n in (-1, 0, 1):
        req.append(case(3, 2, {(0, 1): LEAVERS_MIN + n}, leavers=[n]))
    half = ARR_MAX_WGS * ARR_PER_WG // 2
    req.append(case(3, 3, {(0, 1): half, (2, 0): half + 1}, leavers=None, trips=2))
    return req


def test_table_is_exactly_the_required_cases():
    """every required case is driven by exactly one row, and every row drives a required case: removing, doubling or moving a row off its
    boundary fails here"""
    got = collections.Counter(_signature(r) for r in ROWS)
    want = collections.Counter(_required())
    assert max(want.values()) == 1
    assert got == want, f"missing: {sorted(map(str, want - got))}; not required or doubled: {sorted(map(str, got - want))}"


def test_table_holds_every_threshold_and_either_side():
    """Per threshold the exchange compares a count with: the rows at it and to either side, from the designed positions. Printed."""
    seen = collections.defaultdict(lambda: collections.defaultdict(list))
    for row in ROWS:
        sc = T.build(row)
        part, k = T.part_of(row), row.substeps
        halo_cap, mig_cap, capacity = T.capacities(row, sc)
        lv, held, _ = T.counts(T.facts(part, row.dim, T.designed(sc, k - 2) if k >= 2 else None, T.designed(sc, k - 1)))
        arrivals = [sum(n for (r, f), n in lv.items() if r + (1 if f else -1) == dst) for dst in range(part.world)]
        most = max(max(n.values()) for n in T.needs_over_time(row, sc))
        note = lambda what, value: seen[what][value].append(row.name)
        if mig_cap != GENEROUS and lv:
            note("migrant_capacity - the most leavers of a face", mig_cap - max(lv.values()))
        if halo_cap != GENEROUS:
            note("halo_capacity_records - the most records of a message", halo_cap - most)
            if halo_cap - most <= 0:
                note("a full or overfull table of halo_capacity_records", halo_cap)
        for a in arrivals:
            if a:
                note("arrivals of a slab (ARR_PER_WG = %d; one trip = %d)" % (ARR_PER_WG, ARR_MAX_WGS * ARR_PER_WG), a)
        for n in lv.values():
            note("leavers through one face (a wave of the guests' copy = %d; leavers_cap = %d)" % (WAVE, LEAVERS_MIN), n)
        if row.capacity is not None and min(capacity) < sc["particles"].n:
            note("room - arrivals", min(c - h - a for c, h, a in zip(capacity, held, arrivals)))
    report = []
    for what, values in seen.items():
        report.append(what + ": " + "; ".join(f"{v}: {len(values[v])} rows" + (f" ({', '.join(values[v])})" if len(values[v]) <= 4 else "") for v in sorted(values)))
    print("\n".join(report))
    has = lambda what, vals: set(vals) <= set(next(v for k, v in seen.items() if k.startswith(what)))
    for what in ("migrant_capacity -", "halo_capacity_records -"):          # one short, exactly reached, and room to spare
        assert has(what, (-1, 0)) and max(next(v for k, v in seen.items() if k.startswith(what))) > 0, what
    assert has("a full or overfull table", (1, 2, 3, 4, WAVE - 2, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1, 2 * WAVE + 2))
    assert has("arrivals of a slab", (ARR_PER_WG - 1, ARR_PER_WG, ARR_PER_WG + 1, ARR_MAX_WGS * ARR_PER_WG + 1))
    assert has("leavers through one face", (WAVE - 1, WAVE, WAVE + 1, LEAVERS_MIN - 1, LEAVERS_MIN, LEAVERS_MIN + 1))
    assert has("room -", (-1, 0))
    # the mixed wave: a middle slab whose leavers' list of at most one wave holds both faces
    assert {(1, 1), (5, 3), (31, 33)} <= {(r.leavers.get((1, 0)), r.leavers.get((1, 1))) for r in ROWS if r.world == 3 and r.dim == 3}


def test_parsed_constants_are_the_sources():
    assert (ARR_PER_WG, MIN_INTERIOR_WIDTH, LEAVERS_MIN, LEAVERS_DIV, ARR_MAX_WGS) == (8, 3, 4096, 16, 1024)
    assert MIN_INTERIOR_WIDTH == sharded.MIN_INTERIOR_WIDTH
    assert T.leavers_cap(4096 * 16 + 15) == 4096 and T.leavers_cap(4097 * 16) == 4097
    texts = {"kernels_arrivals.h": "constexpr int ARR_PER_WG = 16;",
             "capi_sharded.inc": "if (has_lower && has_upper && (int64_t)d->dev.shard_hi - (int64_t)d->dev.shard_lo < 4)",
             "capi_lifecycle.inc": "dev.leavers_cap = std::max<uint32_t>(2048u, (uint32_t)(c.particle_capacity / 8));",
             "host_substep.inc": "std::min((arr_most + ARR_PER_WG - 1u) / ARR_PER_WG, 512u)"}
    assert T.constants.__wrapped__(texts) == dict(ARR_PER_WG=16, MIN_INTERIOR_WIDTH=4, LEAVERS_MIN=2048, LEAVERS_DIV=8, ARR_MAX_WGS=512)
    with pytest.raises(AssertionError):
        T.constants.__wrapped__(dict(texts, **{"kernels_arrivals.h": ""}))


def test_a_middle_slab_one_block_too_narrow_is_refused(oracle_libs):
    row = ROW["mig-both-1+1-3d"]
    sc = T.build(row)
    b = T.first_cut(3)
    part = sharded.SlabPartition([b - 64, b, b + MIN_INTERIOR_WIDTH - 1, b + 64])
    assert part.min_interior_width() == MIN_INTERIOR_WIDTH - 1
    sub, gids = split_scene(sc["particles"], part, sc["cell_width"])[1]
    with pytest.raises(AssertionError, match="at least 3 blocks wide"):
        OracleShard(sc, sub, gids, *part.block_range(1), True, True)


# ------------------------------------------------------------------------------------------------ the checks can fail
def _designed_pair(name):
    row = ROW[name]
    sc = T.build(row)
    return row, T.designed(sc, row.substeps - 2), T.designed(sc, row.substeps - 1)


def test_checks_reject_a_halo_rule_without_the_regular_pair(monkeypatch):
    row, pos_a, pos_b = _designed_pair("halo-at-64-3d")
    T.check_facts(row, pos_a, pos_b)
    true_need = T.halo_need
    monkeypatch.setattr(T, "halo_need", lambda *a, **kw: true_need(*a, **dict(kw, regular=False)))
    with pytest.raises(AssertionError, match="halo records"):
        T.check_facts(row, pos_a, pos_b)
    row, pos_a, pos_b = _designed_pair("mig-both-5+3-2d")
    with pytest.raises(AssertionError, match="halo records"):
        T.check_facts(row, pos_a, pos_b)


def test_checks_reject_a_leaver_attributed_to_the_wrong_face(monkeypatch):
    true_leavers = T.leavers
    monkeypatch.setattr(T, "leavers", lambda *a: true_leavers(*a)[::-1])
    for name in ("mig-1-3d", "mig-both-5+3-3d", "mig-both-31+33-2d"):
        row, pos_a, pos_b = _designed_pair(name)
        with pytest.raises(AssertionError, match="leavers"):
            T.check_facts(row, pos_a, pos_b)


def test_checks_reject_a_slab_said_not_to_hold_the_last_leavers(monkeypatch):
    row, pos_a, pos_b = _designed_pair("mig-65-3d")
    part = T.part_of(row)
    holds = [T.held(pos_a, pos_b, part, r, row.dim) for r in range(2)]         # what the slabs export
    T.check_facts(row, pos_a, pos_b, held_ids=holds)
    monkeypatch.setattr(T, "held", lambda pa, pb, part, rank, dim: np.flatnonzero((T.owner(pb, part, dim) == rank) & (T.owner(pa, part, dim) == rank)))
    with pytest.raises(AssertionError, match="held"):
        T.check_facts(row, pos_a, pos_b)
    with pytest.raises(AssertionError, match="holds 71 particles, the truth 6"):
        T.check_facts(row._replace(held=None, halo=None), pos_a, pos_b, held_ids=holds)
