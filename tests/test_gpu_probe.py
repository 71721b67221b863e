"""-m gpu: the Eulerian field output — wgs_sample_grid[_device], wgs_read_grid_window[_device] — against the fp64 truth of
tests/probe_truth.py (its bounds are validated on the CPU by tests/test_probe_truth.py) and against read_grid() of the same handle.

1 every record against the truth on the scenes' own positions, positions jittered over the rim of the active set, every node position
  and the ties of every axis; 2 records do not depend on n or on the order of the points; 3 blocks still in the table but not active
  count as absent; 4 window edges; 5 bad points; 6 before the first substep; 7 the device entry points equal the host forms;
8 asking changes nothing; 9 sharded data is refused."""
import ctypes as C

import numpy as np
import pytest

import probe_truth as PT
import transfer_truth as T
from helpers import assert_same_grid, new_data, pipeline, report_margin, run_gpu
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import SimulationParams

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_samples(tag, data, pts, h, cells, vm, fails):
    s = data.sample_grid(pts)
    tr = PT.Truth(pts, h, cells, vm)
    PT.compare(tag, tr, s.velocity, s.velocity_gradient, s.density, s.active_nodes, fails)
    return s, tr


def _check_window(data, cells, vm, lo, dims):
    vel, mass = data.grid_window(lo, dims)
    evel, emass = PT.dense_window(cells, vm, lo, dims)
    assert vel.shape == evel.shape and mass.shape == emass.shape
    assert np.array_equal(_bits(vel), _bits(evel)) and np.array_equal(_bits(mass), _bits(emass)), ("window", lo, dims)
    return vel, mass


# ------------------------------------------------------------------------------------------------ 1 against the truth
@pytest.mark.parametrize("name,d,h", PT.CASES)
def test_every_record_against_the_truth(hip_libs, name, d, h):
    sc = T.SCENES[name](d, h)
    data = run_gpu(sc, 1)
    cells, vm = data.read_grid()[:2]
    fails = []
    hanging = 0
    for pname, pts in PT.probe_points(sc["particles"].pos, h, cells, seed=d):
        s, tr = _check_samples(f"{name} {d}D h={h}, {pname}", data, pts, h, cells, vm, fails)
        hanging += int(((tr.active_nodes > 0) & (tr.active_nodes < 3 ** d)).sum())
    assert not fails, "\n".join(fails)
    assert hanging > 0, "no stencil hangs over the rim of the active set"


# ------------------------------------------------------------------------------------------------ 2 shape and order
@pytest.mark.parametrize("d", [2, 3])
def test_records_do_not_depend_on_n_or_on_the_order(hip_libs, d):
    h = 0.3
    sc = T.SCENES["ties"](d, h)
    data = run_gpu(sc, 1)
    rng = np.random.default_rng(5 + d)
    pts = rng.uniform(-42 * h, 42 * h, (5000, d)).astype(np.float32)
    whole = data.sample_grid(pts).raw
    assert whole.shape == (5000, d + d * d + 2) and (whole[:, -1] > 0).sum() > 1000
    for n in (0, 1, 63, 64, 65, 257, 5000):
        assert np.array_equal(data.sample_grid(pts[:n]).raw, whole[:n]), n
    perm = rng.permutation(5000)
    assert np.array_equal(data.sample_grid(pts[perm]).raw, whole[perm])


# ------------------------------------------------------------------------------------------------ 3 stale blocks
@pytest.mark.parametrize("d", [2, 3])
def test_blocks_in_the_table_but_not_active_count_as_absent(hip_libs, d):
    """A cube about two blocks wide flies along x at half a cell per substep through free space (no collider, no gravity). Stepped one
    substep at a time; at the first substep where stats() shows blocks in the table that are not active, and again at the first one
    where a cell that was active is no longer, a lattice over the box of every cell seen active so far is sampled and the window of
    that box read. Measured on the MI355X: the condition first holds after substep 2 in both dimensions — the blocks are those the
    fused G2P has already stamped for substep 3 —, and a block the cube left is in the table, inactive, after substep 9 (3D) and 17
    (2D); eviction waits EVICT_AGE = 8 inactive substeps."""
    h = 0.5
    bw = T.bw_of(d)
    rng = np.random.default_rng(40 + d)
    n = 1500 if d == 3 else 800
    pos = rng.uniform((bw + 0.6) * h, (3 * bw - 0.4) * h, (n, d))
    vel = np.zeros((n, d))
    vel[:, 0] = 0.5 * h / T.DT
    sc = T._finish(pos, h, rng, vel=vel, vel_scale=0.0)
    sc["params"] = SimulationParams(gravity=(0.0,) * d, dt=T.DT)
    pipe, data = new_data(sc)
    seen = np.zeros((0, d), np.int64)

    def check_here(tag):
        lo, hi = seen.min(0), seen.max(0)
        # a lattice of two points per cell and axis over the box of every cell seen active so far (and one cell around it)
        axes = [np.arange(2 * (lo[k] - 1), 2 * (hi[k] + 2) + 1) * (0.5 * h) + 0.13 * h for k in range(d)]
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d).astype(np.float32)
        fails = []
        s, tr = _check_samples(tag, data, pts, h, cells, vm, fails)
        assert not fails, "\n".join(fails)
        nothing = tr.active_nodes == 0
        assert nothing.any() and not s.active_nodes[nothing].any() and not s.density[nothing].any() and not s.velocity[nothing].any()
        _check_window(data, cells, vm, lo, hi - lo + 1)
        return pts, nothing

    first = left_at = None
    for step in range(1, 41):
        pipe.step(data, 1)
        data.sync()
        st = data.stats()
        cells, vm = data.read_grid()[:2]
        seen = np.unique(np.concatenate([seen, cells.astype(np.int64)]), axis=0)
        if first is None and st["block_ids"] - st["block_ids_free"] > st["num_active_blocks"]:
            # (the first time this holds, the blocks are those the fused G2P has stamped for the NEXT substep: in the table, stamped
            # with a later epoch than the last executed substep's, and not in its grid)
            first = step
            check_here(f"inactive blocks in the table {d}D, first substep")
        now = set(map(tuple, cells.tolist()))
        left = np.array([c for c in map(tuple, seen.tolist()) if c not in now], np.int64).reshape(-1, d)
        if first is not None and len(left) and st["block_ids"] - st["block_ids_free"] > st["num_active_blocks"]:
            # ... and from here on also the blocks the cube has left: stale, not yet evicted
            left_at = step
            pts, nothing = check_here(f"stale blocks {d}D, first substep after a block was left")
            pc = T.assoc_cell(pts, h) + 1                                # the cell a point's stencil is centred on
            assert (np.isin(T.node_key(pc), T.node_key(left)) & nothing).sum() > 0, "no sample lies in a block the cube left"
            break
    assert first is not None, "in 40 substeps no block was in the table without being active"
    assert left_at is not None, "in 40 substeps the cube left no block"
    report_margin(f"stale blocks {d}D: first substep with inactive blocks in the table", first, 40)
    report_margin(f"stale blocks {d}D: first substep after which a block the cube left is still in the table", left_at, 40)


# ------------------------------------------------------------------------------------------------ 4 window edges
@pytest.mark.parametrize("d", [2, 3])
def test_window_edges(hip_libs, d):
    import torch
    h = 0.5
    sc = T.SCENES["coordinates"](d, h)
    data = run_gpu(sc, 1)
    cells, vm = data.read_grid()[:2]
    bw = T.bw_of(d)
    heavy = cells[int(np.argmax(vm[:, d]))].astype(np.int64)
    vel, mass = _check_window(data, cells, vm, heavy, (1,) * d)                   # one node
    assert mass.reshape(-1)[0] == vm[:, d].max() > 0
    origin = cells[np.abs(cells).max(1) < 4 * bw].astype(np.int64)               # the cluster that straddles 0
    lo = origin.min(0) + np.array([1, 2, 3][:d])
    vel, mass = _check_window(data, cells, vm, lo, (origin.max(0) - origin.min(0) - np.array([2, 5, 4][:d])))   # cuts blocks on every side
    assert (mass > 0).any() and mass.shape[0] % bw != 0
    vel, mass = _check_window(data, cells, vm, (1000,) * d, (3, 4, 5)[:d])        # wholly outside the active set
    assert not _bits(vel).any() and not _bits(mass).any()
    # across the upper end of the key range along x: the cluster two blocks inside it, then 20 cells beyond the last block
    top = (0x8000 if d == 2 else 0x400) * bw + bw - 1                            # last cell inside the range
    corner = cells[np.all(cells > 100 * bw, axis=1)].astype(np.int64)         # the cluster in the all-positive corner
    lo = corner.min(0)
    dims = corner.max(0) - lo + 1
    dims[0] = top + 20 - lo[0]
    vel, mass = _check_window(data, cells, vm, lo, dims)
    assert (mass > 0).any() and not _bits(mass[top - lo[0] + 1:]).any()
    # refused: a zero extent, a product of 2^31 or more; nothing is written
    lib, h_ = data.lib, data._h
    for bad in ((3, 0, 2)[:d], (65536, 32768, 1)[:d], (0xffffffff, 0xffffffff, 0xffffffff)[:d]):
        out = np.full(64, 7.0, np.float32)
        lo32 = (C.c_int32 * d)()
        st = lib.wgs_read_grid_window(h_, lo32, (C.c_uint32 * d)(*bad), out.ctypes.data_as(C.POINTER(C.c_float)))
        assert st == INVALID and lib.wgs_last_error() and (out == 7.0).all(), bad
        dev = torch.full((64,), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(_ffi.WgsError) as e:
            data.grid_window_device((0,) * d, bad, dev.data_ptr())
        assert e.value.code == INVALID
        data.sync()
        assert (dev.cpu().numpy() == 7.0).all(), bad


# ------------------------------------------------------------------------------------------------ 5 bad points
@pytest.mark.parametrize("d", [2, 3])
def test_bad_points_give_zero_records_and_leave_the_others_alone(hip_libs, d):
    h = 0.5
    sc = T.SCENES["coordinates"](d, h)
    data = run_gpu(sc, 1)
    cells, vm = data.read_grid()[:2]
    bw = T.bw_of(d)
    good = sc["particles"].pos[:200].copy()
    bad = []
    for k in range(d):
        for v in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            p = good[len(bad)].copy()
            p[k] = v
            bad.append(p)
    edge, edge_bad = [], []
    for k in range(d):
        top = (0x8000 if d == 2 else (0x200 if k == 1 else 0x400)) * bw * h      # first cell of the last block inside the range
        for off, is_bad in ((1.0, False), (bw - 1.4, True), (bw - 0.4, True), (bw + 1.0, True), (bw + 40.0, True)):
            p = np.zeros(d, np.float32)
            p[k] = top + off * h
            edge.append(p)
            edge_bad.append(is_bad)
    bot = -(0x7fff if d == 2 else 0x3ff) * bw * h                                # first cell of the first block inside, along x
    for off, is_bad in ((1.0, False), (-0.6, True), (-3.0, True)):
        p = np.zeros(d, np.float32)
        p[0] = bot + off * h
        edge.append(p)
        edge_bad.append(is_bad)
    expect_bad = np.array([True] * len(bad) + edge_bad)
    special = np.concatenate([np.array(bad, np.float32), np.array(edge, np.float32)])
    assert np.array_equal(PT.bad_points(special, h), expect_bad)
    alone = data.sample_grid(good).raw
    # interleaved, so that good and bad points share waves
    mixed = np.concatenate([good, special])
    order = np.random.default_rng(d).permutation(len(mixed))
    got = data.sample_grid(mixed[order]).raw
    back = np.empty_like(got)
    back[order] = got
    assert np.array_equal(back[:len(good)], alone), "a good point's record changed with bad points in the call"
    assert not back[len(good):][expect_bad].any(), "a bad point's record is not all zero"
    fails = []
    _check_samples(f"bad points {d}D, the others", data, mixed, h, cells, vm, fails)
    assert not fails, "\n".join(fails)
    data.sync()                                                                   # (no device error was left behind)
    assert data.stats()["overflow"] == 0


# ------------------------------------------------------------------------------------------------ 6 before the first substep
@pytest.mark.parametrize("d", [2, 3])
def test_before_the_first_substep_everything_is_zero(hip_libs, d):
    sc = T.SCENES["ties"](d, 0.5)
    _, data = new_data(sc)
    s = data.sample_grid(sc["particles"].pos)
    assert not s.raw.any()
    vel, mass = data.grid_window((-8,) * d, (16,) * d)
    assert not _bits(vel).any() and not _bits(mass).any()
    assert data.sample_grid(np.zeros((0, d), np.float32)).raw.shape == (0, d + d * d + 2)


# ------------------------------------------------------------------------------------------------ 7 entry points agree
@pytest.mark.parametrize("d", [2, 3])
def test_device_entry_points_equal_the_host_forms(hip_libs, d):
    import torch
    h = 0.3
    sc = T.SCENES["ties"](d, h)
    data = run_gpu(sc, 3)
    rng = np.random.default_rng(9)
    pts = rng.uniform(-42 * h, 42 * h, (3001, d)).astype(np.float32)
    host = data.sample_grid(pts).raw
    words = d + d * d + 2
    dpts = torch.from_numpy(pts).to("cuda:0")
    dout = torch.full((len(pts) * words,), -1, dtype=torch.int32, device="cuda:0")
    lo, dims = (-20,) * d, (37, 41, 29)[:d]
    hvel, hmass = data.grid_window(lo, dims)
    dwin = torch.full((int(np.prod(dims)) * (d + 1),), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    data.sample_grid_device(dpts.data_ptr(), len(pts), dout.data_ptr())
    data.grid_window_device(lo, dims, dwin.data_ptr())
    data.sample_grid_device(dpts.data_ptr(), 0, dout.data_ptr())                  # n == 0: OK, writes nothing
    data.sync()
    assert dout.cpu().numpy().view(np.uint32).tobytes() == host.tobytes()
    win = dwin.cpu().numpy().reshape(tuple(dims[::-1]) + (d + 1,)).transpose(tuple(range(d - 1, -1, -1)) + (d,))
    assert win[..., :d].tobytes() == hvel.tobytes() and np.ascontiguousarray(win[..., d]).tobytes() == hmass.tobytes()
    assert (hmass > 0).any() and host[:, -1].any()


# ------------------------------------------------------------------------------------------------ 8 asking changes nothing
def _stirred(d):
    rng = np.random.default_rng(60 + d)
    bw, h = T.bw_of(d), 0.3
    n = 3000 if d == 3 else 1500
    pos = rng.uniform(2 * bw * h, 5 * bw * h, (n, d))
    c = pos.mean(0)
    vel = np.zeros((n, d))
    vel[:, 0], vel[:, 1] = -(pos[:, 1] - c[1]), pos[:, 0] - c[0]
    vel = vel * (40.0 / (1.5 * bw)) + rng.normal(0.0, 10.0 * h, (n, d))
    return T._finish(pos, h, rng, vel=vel)


@pytest.mark.parametrize("kind", ["stirred2", "stirred3", "sand3"])
def test_asking_changes_nothing(hip_libs, kind):
    import torch
    sc = scenes.reference_sand3() if kind == "sand3" else _stirred(int(kind[-1]))
    d, h = sc["particles"].dim, sc["cell_width"]

    def end_state(ask):
        pipe, data = new_data(sc)
        pipe.step(data, 10)
        if ask:
            pts = sc["particles"].pos[::7].copy()
            lo, dims = (-4,) * d, (40,) * d
            s = data.sample_grid(pts)
            assert s.active_nodes.any() and np.isfinite(s.velocity).all() and (s.density >= 0).all()
            vel, mass = data.grid_window(lo, dims)
            dpts = torch.from_numpy(pts).to("cuda:0")
            dout = torch.zeros(len(pts) * (d + d * d + 2), dtype=torch.int32, device="cuda:0")
            dwin = torch.zeros(40 ** d * (d + 1), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            data.sample_grid_device(dpts.data_ptr(), len(pts), dout.data_ptr())
            data.grid_window_device(lo, dims, dwin.data_ptr())
        pipe.step(data, 10)
        data.sync()
        out = data.diagnostics(_ffi.DIAG_ALL).raw, data.read_grid(), data.stats()["num_active_blocks"]
        data.close()
        return out

    asked, plain = end_state(True), end_state(False)
    assert asked[0] == plain[0], "diagnostics differ"
    assert_same_grid(asked[1], plain[1])
    assert asked[2] == plain[2]


# ------------------------------------------------------------------------------------------------ 9 sharded data
@pytest.mark.parametrize("d", [2, 3])
def test_sharded_data_is_refused(hip_libs, d):
    import torch
    sc = _stirred(d)
    pipe = pipeline(d)
    shards, _ = lockstep_slabs(pipe, sc, 2)
    lib, T_ = pipe.lib, pipe.T
    pts = np.zeros((4, d), np.float32)
    out = (T_.GridSample * 4)()
    lo, dims = (C.c_int32 * d)(), (C.c_uint32 * d)(*([2] * d))
    win = np.full(2 ** d * (d + 1), 7.0, np.float32)
    dev = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    fp = C.POINTER(C.c_float)
    for s in shards:
        calls = [lambda: lib.wgs_sample_grid(s._h, pts.ctypes.data_as(fp), 4, out),
                 lambda: lib.wgs_sample_grid_device(s._h, C.c_void_p(dev.data_ptr()), 4, C.c_void_p(dev.data_ptr())),
                 lambda: lib.wgs_read_grid_window(s._h, lo, dims, win.ctypes.data_as(fp)),
                 lambda: lib.wgs_read_grid_window_device(s._h, lo, dims, C.c_void_p(dev.data_ptr()))]
        for call in calls:
            assert call() == UNSUPPORTED
            assert b"sharded" in lib.wgs_last_error()
    assert (win == 7.0).all() and not bytes(out).strip(b"\0")
    for s in shards:
        s.close()
