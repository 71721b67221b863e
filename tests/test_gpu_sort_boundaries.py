"""The regrouping of a block (kernels_sort.h, launch 2) and the binning of a rebuild substep (bin_body) at every threshold the kernel compares
a count with, at the threshold's exact value and one to either side: one case per row of sort_truth.ROWS.

A case steps K - 2 substeps and reads `pos_a`, one more and reads `pos_b`, then the checked substep, whose sort orders `pos_b` and meets the
motion pos_a -> pos_b. From the positions the GPU run itself read back:
  * sort_truth.paths of the row's block equals the row's designed counts and predicate outcomes, with == (a scene that drifted off its boundary
    fails here and says so);
  * the runs are in canonical order (gpu_common.assert_canonical_order) and hold the particles the fp32 oracle stepped alongside puts in each
    block (gpu_common.check_blocks); nothing overflowed; the table was rebuilt by the checked substep on the rebuild rows and on no other;
  * stats()["cell_changers"] grew over the checked substep by the number of particles whose associated cell differs between pos_a and pos_b.
    That is what the kernel counts: regroup_block returns, in the wave-parallel form, the staged entries of the previous run flagged
    CELL_MOVED whose new cell lies in the block plus the array arrivals, and in the lane-by-lane form the sum of the cells' arrivals
    (handed over inside the block, from the block's array, from the cells' lists) — every particle that changed cell, counted once, in the
    block it is in now; a rebuild substep counts nothing;
  * after the checked substep positions and velocities agree with the fp32 oracle within gpu_common.PART_TOL (relative RMS: the project's
    one-substep tolerance) — a particle dropped from a run takes no part in P2G / G2P and fails here too;
  * the same case under WGS_DEBUG CELL_INSERTION_SORT (an independent ordering of the same cells) leaves the same runs block by block, and
    under NO_DIRECT_RUNS the same runs and the same BASE_FIELDS bit for bit."""
import numpy as np
import pytest

from wgsparkl_amd.selfcheck import rel_rms

from helpers import BASE_FIELDS, assert_same_bits, debug, new_data, oracle
from gpu_common import PART_TOL, assert_canonical_order, check_blocks
import sort_truth as S
from sort_truth import ROW


def _run(row, checked):
    """the row's case on the GPU; `checked`: with the oracle alongside and every check of the docstring (else only the order and the state)"""
    sc = S.build(row)
    ps = sc["particles"]
    k = row.substeps
    pipe, data = new_data(sc)
    st = None
    if checked:
        st = oracle(ps.dim, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    pos_a, pos_b = None, ps.pos
    if k > 1:
        pipe.step(data, k - 2)
        data.sync()
        pos_a = data.read_particles().pos
        pipe.step(data, 1)
        data.sync()
        pos_b = data.read_particles().pos
        if checked:
            st.step(k - 1)
    s0 = data.stats()
    pipe.step(data, 1)
    data.sync()
    s1 = data.stats()
    vid, first, num, ids = assert_canonical_order(data, pos_b, ps.dim, S.H)
    got = data.read_particles()
    runs = {tuple(v): ids[f:f + n].tolist() for v, f, n in zip(vid.tolist(), first.tolist(), num.tolist())}
    if not checked:
        return runs, got
    f = S.check_paths(row, pos_a, pos_b)
    st.step(1)
    assert not st.overflow
    check_blocks(data, st)
    assert s1["overflow"] == 0
    rebuilt = s1["table_rebuilds"] - s0["table_rebuilds"]
    changed = s1["cell_changers"] - s0["cell_changers"]
    if k > 1:
        assert rebuilt == 0, "the checked substep rebuilt the table: not a steady-state substep"
        want = int((f["cell_a"] != f["cell_b"]).any(1).sum())
        print(f"{row.name}: cell_changers grew by {changed}, {want} particles changed cell")
        assert changed == want
    else:
        assert rebuilt == 1 and changed == 0
    for name in ("pos", "vel"):
        err = rel_rms(getattr(got, name), st.arr[name])
        print(f"{row.name}: {name} rel rms vs the fp32 oracle {err:.3e} (bound {PART_TOL:.0e})")
        assert err < PART_TOL, (name, err)
    return runs, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROW))
def test_boundary_case(hip_libs, monkeypatch, name):
    row = ROW[name]
    runs, got = _run(row, checked=True)
    with debug(monkeypatch, "CELL_INSERTION_SORT"):
        runs_ins, _ = _run(row, checked=False)
    assert runs_ins == runs, "the insertion sort orders the same cells differently"
    with debug(monkeypatch, "NO_DIRECT_RUNS"):
        runs_nd, got_nd = _run(row, checked=False)
    assert runs_nd == runs
    assert_same_bits(got, got_nd, BASE_FIELDS, "NO_DIRECT_RUNS")
