"""CPU twins of tests/test_gpu_sort_boundaries.py: every row of sort_truth.ROWS stepped with the fp32 oracle meets exactly the counts and
predicate outcomes it was designed for; the table covers every threshold at its value and one to either side; `paths` gives the spelled-out
outcomes of two hand-written position pairs; the parsed constants are the kernel's; and the checks the GPU file applies reject an orderer
that drops the last entry of a full run, misplaces the fifth newcomer of a cell, or keeps the arrival behind the block's array in it."""
import collections
import re

import numpy as np
import pytest

from oracle.np_oracle import assoc_cell, bw_of
from helpers import oracle
from gpu_common import assert_runs_canonical
import sort_truth as S
from sort_truth import ARRC, BLK_ARR, HALF, NEWC, PAR_R, ROW, ROWS, RUNCAP, SORT_THREADS, TOUCH_SET


def oracle_positions(row, sc):
    """(pos_a, pos_b, state after the checked substep) of the row's scene on the fp32 oracle"""
    ps = sc["particles"]
    st = oracle(ps.dim, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    pos_a, pos_b = None, ps.pos
    if row.substeps > 1:
        st.step(row.substeps - 2)
        pos_a = st.arr["pos"].copy()
        st.step(1)
        pos_b = st.arr["pos"].copy()
    st.step(1)
    assert not st.overflow
    return pos_a, pos_b, st


@pytest.mark.parametrize("name", list(ROW))
def test_row_meets_its_designed_counts_on_the_oracle(oracle_libs, name):
    row = ROW[name]
    sc = S.build(row)
    assert sc["particles"].n <= 1600 and sc["particles"].dim == row.dim
    pos_a, pos_b, _ = oracle_positions(row, sc)
    S.check_paths(row, pos_a, pos_b)


def _designed(row):
    """paths() of the row's block from positions made by pure translation (no oracle): what the coverage is computed from"""
    sc = S.build(row)
    ps = sc["particles"]
    step = ps.vel.astype(np.float64) * S.DT
    pos_a = pos_b = None
    if row.substeps > 1:
        pos_a = (ps.pos + (row.substeps - 2) * step).astype(np.float32)
        pos_b = (ps.pos + (row.substeps - 1) * step).astype(np.float32)
    else:
        pos_b = ps.pos
    return S.paths(S.facts(pos_a, pos_b, row.dim), S.block_of(row))


def test_table_holds_every_threshold_and_one_to_either_side():
    """For every threshold predicate: rows that name it, in 3D, at the threshold, one below and one above — with the predicate's outcome
    differing across the threshold where it is the row's to decide; the round tail at 63, 0 and 1 entries past a full round; TOUCH_SET at
    31, 32 and 33 blocks; and the 2D rows the block-level predicates and each per-cell kind need. Prints each predicate with its values. (That no single row can go: the test after this one.)"""
    seen = {k: set() for k in S.THRESHOLDS}
    seen2d = {k: set() for k in S.THRESHOLDS}
    tails, touch, touch2d = set(), set(), set()
    for row in ROWS:
        if row.wg is not None:
            (touch if row.dim == 3 else touch2d).update((n, len(row.wg)) for n in row.wg)
            continue
        p = _designed(row)
        cell = row.cell[0] if row.cell is not None else 0
        for name in row.predicates:
            if name in S.THRESHOLDS:
                value = S.THRESHOLDS[name][0](p, cell)
                if value is not None:
                    (seen if row.dim == 3 else seen2d)[name].add(value)
        if "tail" in row.predicates and row.dim == 3:
            tails.add((p.runlen, p.narr))
    report = []
    for name, (_, thr) in S.THRESHOLDS.items():
        report.append(f"{name}: threshold {thr}, 3D rows at {sorted(seen[name])}, 2D rows at {sorted(seen2d[name])}")
        assert {thr - 1, thr, thr + 1} <= seen[name], report[-1]
        assert {thr, thr + 1} <= seen2d[name], report[-1]
    print("\n".join(report))
    assert {(r, a) for r in (1, 63, 64, 65, 128, 129) for a in (0, 1)} <= tails
    assert {(n, w) for n in (TOUCH_SET - 1, TOUCH_SET, TOUCH_SET + 1) for w in (1, 2)} <= touch and (TOUCH_SET + 1, 1) in touch2d
    names = {r.name for r in ROWS}
    for dim in (3, 2):      # the rows no threshold set above accounts for
        for n in ("in_lds-above-out-below", "par-sum-at-but-listed", "clean-1", f"clean-{BLK_ARR}", f"clean-{BLK_ARR + 1}", "all-leave-to-plus",
                  "all-leave-to-minus", "rebuild-block-at", "rebuild-block-above", f"array-{BLK_ARR + 1}-over-2"):
            assert f"{n}-{dim}d" in names, n
    for n in (1, ARRC, ARRC + 1, 64, 65):
        assert f"rebuild-cell-{n}-3d" in names
    # target cells: the first and the last lane both occur, in the parallel and in the lane form
    for kind in ("NEWC", "coop"):
        assert {0, 24, 63} <= {r.cell[0] for r in ROWS if kind in r.predicates and r.dim == 3}
    # the newcomers of the parallel form, with and without stayers: every (same, other) split the issue lists
    for st in (5, 0):
        got = {(r.cell[1]["new_same"], r.cell[1]["new_other"]) for r in ROWS if "NEWC" in r.predicates and r.dim == 3 and r.cell[1]["stayed"] == st and r.cell[0] == 24}
        assert {(3, 0), (4, 0), (0, 4), (2, 2), (5, 0), (0, 5), (3, 2)} <= got


def _signature(row):
    """what a row drives, from its designed positions alone (not from its name or its expectations)"""
    if row.wg is not None:
        pos = S.build(row)["particles"].pos
        b = assoc_cell(pos, S.H) // bw_of(row.dim)
        last = (b[:, 0] == b[:, 0].max())[:SORT_THREADS]          # where the last block's particles sit in the first workgroup
        where = "first" if last[:4].all() else "last" if last[-4:].all() else "mixed"
        return ("touch", row.dim, tuple(S.workgroup_blocks(pos, row.dim)), where)
    p = _designed(row)
    kind = "rebuild" if row.substeps == 1 else row.block
    sig = (kind, row.dim, p.runlen, p.narr, p.btotal, p.dirty, int(np.count_nonzero(p.new_other)) if kind == "target" else 0)
    if kind == "source":
        sig += (S.block_of(row)[0] - S.target_block(row.dim)[0],)
    if row.last_change:
        sig += ("last entries change",)
    if row.cell is not None:
        c = row.cell[0]
        sig += (c, int(p.stayed[c]), int(p.new_same[c]), int(p.new_other[c]), "par" if p.par else "lane")
    return sig


def _required():
    """the minimum cases, written out from the constants: block-level rows in both dimensions, per-cell rows in 3D and one of each kind in 2D"""
    R, B, A4 = RUNCAP, BLK_ARR, ARRC
    req = []
    for d in (3, 2):
        blk = lambda r, a, tot, dirty=True, cells=None: ("target", d, r, a, tot, dirty, (1 if a else 0) if cells is None else cells)
        req += [blk(R - 1, 0, R - 1), blk(R, 0, R), blk(R + 1, 0, R + 1), blk(R + 1, 0, R - 1)]                               # in_lds
        req += [blk(R - 1, 1, R), blk(R, 1, R + 1), blk(R - B, B, R), blk(R - B + 1, B, R + 1), blk(R - B - 1, B + 1, R)]     # par, out_lds
        req += [blk(300, a, 300 + a, cells=c) for a in (B - 1, B, B + 1) for c in (1, 2)]                                     # array against list
        req += [blk(r, 0, r) + ("last entries change",) for r in (HALF - 1, HALF, HALF + 1)]                                  # second batch
        req += [blk(r, a, r + a) for r in (1, 63, 64, 65, 128, 129) for a in (0, 1)]                                          # round tail
        req += [blk(300, a, 300 + a, dirty=False) for a in (1, B, B + 1)]                                                     # clean, arrivals only
        req += [("source", d, 40, 0, 0, True, 0, side) for side in (-1, 1)]                                                   # everybody leaves
        req += [("rebuild", d, 0, 0, R, False, 0), ("rebuild", d, 0, 0, R + 1, False, 0)]
        cell = lambda r, a, tot, c, st, same, other, form, cells=None: blk(r, a, tot, cells=cells) + (c, st, same, other, form)
        splits = ((3, 0), (4, 0), (0, 4), (2, 2), (5, 0), (0, 5), (3, 2)) if d == 3 else ((4, 0), (3, 2))
        req += [cell(200, o, 200 + o, 24, st, s, o, "par") for st in (5, 0) for s, o in splits]                               # NEWC
        req += [cell(200, 2, 202, c, 5, s, 2, "par") for c in (0, 63) for s in ((2, 3) if d == 3 else (3,))]
        for n in ((A4 - 1, A4, A4 + 1) if d == 3 else (A4, A4 + 1)):                                                          # ARRC, lane form
            req += [cell(200, B + 1, 200 + B + 1, 24, 5, n, 0, "lane"), cell(R - 2, n, R - 2 + n, 24, 5, 0, n, "lane")]
        for tot, c in ((63, 24), (64, 24), (65, 24)) + (((64, 0), (64, 63)) if d == 3 else ()):                              # cell total against 64
            req += [cell(300, B + 3, 300 + B + 3, c, tot - 5, 3, 2, "lane", cells=2)]
        for n in ((1, A4, A4 + 1, 64, 65) if d == 3 else (A4 + 1, 65)):                                                       # rebuild, per cell
            req += [("rebuild", d, 0, 0, n + 130, False, 0, 24, 0, 0, n, "lane")]
    for w in (1, 2):
        req += [("touch", 3, (n,) * w, "last") for n in (TOUCH_SET - 1, TOUCH_SET, TOUCH_SET + 1)]
        req += [("touch", 3, (TOUCH_SET + 1,) * w, o) for o in ("first", "mixed")] + [("touch", 2, (TOUCH_SET + 1,) * w, "last")]
    return req


def test_table_is_exactly_the_required_cases():
    """every required case is driven by exactly one row, and every row drives a required case: removing, doubling or moving a row fails here"""
    got = collections.Counter(_signature(r) for r in ROWS)
    want = collections.Counter(_required())
    assert max(want.values()) == 1
    assert got == want, f"missing: {sorted(map(str, want - got))}; not required or doubled: {sorted(map(str, got - want))}"


def _pair(dim, before, after):
    """positions in the middle of the given world cells"""
    f = lambda cells: (np.asarray(cells, np.float64) + 1.0).astype(np.float32)
    return S.facts(f(before), f(after), dim)


def test_paths_on_two_hand_written_pairs():
    # 3D, block (3, 2, 2) = cells x 12..15, y 8..11, z 8..11. Six particles:
    #   0, 1  stay in cell (12, 8, 8), local 0
    #   2     (12, 8, 8) -> (13, 8, 8): changes cell inside the block, local 0 -> 1
    #   3     (11, 8, 8) -> (12, 8, 8): arrives from block (2, 2, 2) in local 0
    #   4     (15, 11, 11) -> (16, 11, 11): leaves local 63 for block (4, 2, 2)
    #   5     stays in (15, 11, 11), local 63
    a = [(12, 8, 8), (12, 8, 8), (12, 8, 8), (11, 8, 8), (15, 11, 11), (15, 11, 11)]
    b = [(12, 8, 8), (12, 8, 8), (13, 8, 8), (12, 8, 8), (16, 11, 11), (15, 11, 11)]
    p = S.paths(_pair(3, a, b), (3, 2, 2))
    assert (p.runlen, p.narr, p.btotal, p.dirty, p.tail) == (5, 1, 5, True, 5)
    assert (p.in_lds, p.par, p.out_lds, p.second_half, p.on_lists) == (True, True, True, False, False)
    assert (p.stayed[0], p.new_same[0], p.new_other[0], p.total[0]) == (2, 0, 1, 3)
    assert (p.stayed[1], p.new_same[1], p.new_other[1], p.total[1]) == (0, 1, 0, 1)
    assert (p.stayed[63], p.new_same[63], p.new_other[63], p.total[63]) == (1, 0, 0, 1)
    assert p.total.sum() == 5 and p.network.all() and not (p.cached.any() or p.coop.any() or p.select.any())
    q = S.paths(_pair(3, a, b), (4, 2, 2))       # the block the leaver enters: no previous run, one arrival, in its local cell 0 + 12 + 48
    assert (q.runlen, q.narr, q.btotal, q.dirty, q.par) == (0, 1, 1, False, True) and q.new_other[60] == 1
    q = S.paths(_pair(3, a, b), (2, 2, 2))       # the block the arrival left: a run of one, nobody in it any more
    assert (q.runlen, q.narr, q.btotal, q.dirty) == (1, 0, 0, True) and q.total.sum() == 0
    # 2D, block (2, 2) = cells 16..23 x 16..23; 70 particles arrive from block (1, 2) in local cell 0 + (3 << 3), which holds 2 stayers; 5 more
    # change from local cell 1 to local cell 1 + (1 << 3), inside the block
    a = [(16, 19)] * 2 + [(15, 19)] * 70 + [(17, 16)] * 5
    b = [(16, 19)] * 2 + [(16, 19)] * 70 + [(17, 17)] * 5
    p = S.paths(_pair(2, a, b), (2, 2))
    assert (p.runlen, p.narr, p.btotal, p.dirty, p.tail) == (7, 70, 77, True, 7)
    assert (p.in_lds, p.par, p.out_lds, p.second_half, p.on_lists) == (True, False, True, False, True)     # 70 > BLK_ARR: six are on the cell's list
    assert (p.stayed[24], p.new_same[24], p.new_other[24], p.total[24]) == (2, 0, 70, 72)
    assert (p.stayed[9], p.new_same[9], p.new_other[9], p.total[9]) == (0, 5, 0, 5)
    assert p.select[24] and not p.coop[24] and p.coop[9] and not p.cached[9] and p.cached[0]
    # the same positions as a first substep: no previous run, everybody on a list
    r = S.paths(S.facts(None, (np.asarray(b, np.float64) + 1.0).astype(np.float32), 2), (2, 2))
    assert (r.runlen, r.narr, r.btotal, r.dirty, r.par, r.on_lists) == (0, 0, 77, False, False, True) and r.new_other[24] == 72 and r.select[24]


def test_parsed_constants_are_the_kernels():
    assert (RUNCAP, BLK_ARR, ARRC, NEWC, TOUCH_SET, SORT_THREADS, S.NPB) == (768, 64, 4, 4, 32, 256, 64)
    assert PAR_R == (RUNCAP + 63) // 64 and HALF == 64 * (PAR_R // 2)
    # what the kernel's own static_asserts and aliases rest on, restated
    assert PAR_R % 2 == 0 and RUNCAP <= 1023 and RUNCAP >= 64 + 2 * 64 * ARRC
    # the parser follows the text, not a table of its own
    text = "constexpr int RUNCAP = 512;\nconstexpr uint32_t BLK_ARR = 32u;\nconstexpr int ARRC = 4; constexpr int NEWC = 4;\n" \
           "constexpr int PAR_R = (RUNCAP + 63) / 64;\nconstexpr int TOUCH_SET = 16; constexpr int SORT_THREADS = 256; constexpr int NPB = 64;"
    got = S.constants(text)
    assert (got["RUNCAP"], got["BLK_ARR"], got["PAR_R"], got["TOUCH_SET"]) == (512, 32, 8, 16)
    with pytest.raises(AssertionError):
        S.constants(re.sub(r"constexpr int ARRC = 4;", "", text))


# ---- the checks of the GPU file against an orderer with a fault injected (the CPU twin of the orderer: sort_truth._lexsorted_runs)
def _runs_of(name):
    row = ROW[name]
    sc = S.build(row)
    pos_a, pos_b, st = oracle_positions(row, sc)
    vid, first, num, ids = S._lexsorted_runs(pos_b, row.dim)
    assert_runs_canonical(vid, first, num, ids, pos_b, row.dim, S.H)
    b = int(np.flatnonzero((vid == np.asarray(S.block_of(row))).all(1))[0])
    return row, pos_a, pos_b, vid, first, num, ids.copy(), b


def test_checks_reject_a_full_run_without_its_last_entry(oracle_libs):
    row, _, pos_b, vid, first, num, ids, b = _runs_of("in_lds-at-3d")
    assert num[b] == RUNCAP
    last = first[b] + num[b] - 1
    lost = ids[last]
    ids[last] = ids[last - 1]                 # the slot behind a run that is exactly full was never written: it holds what was there
    with pytest.raises(AssertionError):
        assert_runs_canonical(vid, first, num, ids, pos_b, row.dim, S.H)
    short = num.copy()                        # ... or the run is one short
    short[b] -= 1
    with pytest.raises(AssertionError):
        assert_runs_canonical(vid, first, short, np.delete(ids, last), pos_b, row.dim, S.H)
    assert lost not in np.delete(ids, last)


def test_checks_reject_a_misplaced_fifth_newcomer(oracle_libs):
    row, pos_a, pos_b, vid, first, num, ids, b = _runs_of("newc-5+3+2-3d")
    bw = bw_of(row.dim)
    ca, cb = assoc_cell(pos_a, S.H), assoc_cell(pos_b, S.H)
    run = ids[first[b]:first[b] + num[b]]
    members = np.flatnonzero(S.local_key(cb[run], row.dim) == row.cell[0])
    assert len(members) == 10
    new = [m for m in members if (ca[run[m]] != cb[run[m]]).any()]
    assert len(new) == NEWC + 1
    # the register network orders NEWC newcomers; the fifth left where the counting sort dropped it — behind the cell's other members
    fifth = new[2]
    assert fifth != members[-1], "the newcomer must rank among the cell's members for the fault to show"
    order = [m for m in members if m != fifth] + [fifth]
    bad = ids.copy()
    bad[first[b] + members] = run[order]
    with pytest.raises(AssertionError):
        assert_runs_canonical(vid, first, num, bad, pos_b, row.dim, S.H)


def test_checks_reject_an_arrival_written_behind_the_blocks_array(oracle_libs):
    """65 arrivals, all 65 sent to the array of 64: the 65th lands in the first entry of the next block's array and on no list — it is in
    nobody's run, or, where the next block reads it, in the wrong block's."""
    row, pos_a, pos_b, vid, first, num, ids, b = _runs_of(f"array-{BLK_ARR + 1}-over-1-3d")
    bw = bw_of(row.dim)
    ca, cb = assoc_cell(pos_a, S.H), assoc_cell(pos_b, S.H)
    run = ids[first[b]:first[b] + num[b]]
    arrived = [m for m in range(len(run)) if (ca[run[m]] // bw != cb[run[m]] // bw).any()]
    assert len(arrived) == BLK_ARR + 1
    at = first[b] + arrived[-1]
    short = num.copy()
    short[b] -= 1
    with pytest.raises(AssertionError):        # in nobody's run
        assert_runs_canonical(vid, first, short, np.delete(ids, at), pos_b, row.dim, S.H)
    other = (b + 1) % len(vid)                 # in the next block's run
    moved = np.insert(np.delete(ids, at), first[other] - (1 if other > b else 0), ids[at])
    n2 = short.copy()
    n2[other] += 1
    f2 = np.concatenate([[0], np.cumsum(n2)[:-1]])
    with pytest.raises(AssertionError):
        assert_runs_canonical(vid, f2, n2, moved, pos_b, row.dim, S.H)
    # and paths itself says the 65th is on a list, not in the array
    assert S.paths(S.facts(pos_a, pos_b, row.dim), S.block_of(row)).on_lists
