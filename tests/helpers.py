"""Shared helpers of the parity tests: run the same scene through the CPU oracle
(fp32 restatement + fp64 "truth") and through the HIP path (C ABI), then compare
by VIRTUAL ids (world cell coordinates), never by physical node index."""
import contextlib
import dataclasses
import functools
import os
import re

import numpy as np

from oracle.orc import Oracle
from wgsparkl_amd import MpmData, MpmPipeline, _ffi
from wgsparkl_amd.selfcheck import rel_rms

_ORACLES = {}
_LAYOUT_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wgsparkl_amd", "csrc", "layout.h")


@functools.lru_cache(maxsize=None)
def _debug_bits():
    with open(_LAYOUT_H) as f:
        return {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"^\s*DBG_(\w+) = 1u << (\d+),", f.read(), re.M)}


def debug_switches(*names):
    """The WGS_DEBUG value that turns on the named developer switches: the DBG_* bits of layout.h, named without the prefix."""
    bits = _debug_bits()
    value = 0
    for name in names:
        value |= bits[name]
    return str(value)


@contextlib.contextmanager
def debug(monkeypatch, *names):
    """WGS_DEBUG = debug_switches(*names) inside the block; what was there before (a value, or nothing) after it."""
    with monkeypatch.context() as m:
        m.setenv("WGS_DEBUG", debug_switches(*names))
        yield


def oracle(dim, dtype):
    key = (dim, np.dtype(dtype).name)
    if key not in _ORACLES:
        _ORACLES[key] = Oracle(dim, dtype)
    return _ORACLES[key]


def run_oracle(scene, nsteps, dtype=np.float32):
    ps = scene["particles"]
    st = oracle(ps.dim, dtype).new_state(ps, scene["params"], scene["colliders"], scene["cell_width"],
                                         scene["grid_capacity"], scene.get("model", 0))
    st.step(nsteps)
    assert not st.overflow
    return st


_PIPES = {}


def pipeline(dim):
    if dim not in _PIPES:
        _PIPES[dim] = MpmPipeline(0, dim)
    return _PIPES[dim]


def new_data(scene, **overrides):
    """(pipeline, data) of a scene on the shared pipeline of its dimension; `overrides` as in MpmData.from_scene."""
    pipe = pipeline(overrides.get("particles", scene["particles"]).dim)
    return pipe, MpmData.from_scene(pipe, scene, **overrides)


def step_chunks(scene_or_data, chunks, timestamps=False):
    """One wgs_step call per entry of `chunks` with a wgs_sync after each, on existing data or on new data of a scene; returns the data."""
    data = new_data(scene_or_data)[1] if isinstance(scene_or_data, dict) else scene_or_data
    for k in chunks:
        data.pipeline.step(data, k, timestamps)
        data.sync()
    return data


def run_gpu(scene, nsteps, timestamps=False):
    return step_chunks(scene, (nsteps,), timestamps)


# the read_particles() fields the bit-identity tests compare: the state a substep advances, + the affinity word of collider scenes,
# + the plastic state, + the rest of the particle cdf
BASE_FIELDS = ("pos", "vel", "def_grad", "affine")
AFFINITY_FIELDS = BASE_FIELDS + ("cdf_affinity",)
PLASTIC_FIELDS = AFFINITY_FIELDS + ("dp_state",)
CDF_FIELDS = PLASTIC_FIELDS + ("cdf_normal", "cdf_dist")


def assert_same_bits(a, b, fields, tag=None):
    """np.array_equal field by field: -0.0 equals 0.0 and a NaN equals nothing, itself included."""
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f if tag is None else (tag, f)


def assert_same_grid(ga, gb):
    """two read_grid() tuples"""
    assert len(ga) == len(gb), (len(ga), len(gb))
    for k, (x, y) in enumerate(zip(ga, gb)):
        assert np.array_equal(x, y), ("grid", k)


def assert_same_bodies(ba, bb, keys=None):
    """two read_body_poses() lists, by `keys` (default: every key of the first list's dicts)"""
    assert len(ba) == len(bb), (len(ba), len(bb))
    for i, (x, y) in enumerate(zip(ba, bb)):
        for key in (x if keys is None else keys):
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), (i, key)


def restored_colliders(colliders, bodies, dim):
    """The colliders a restarted run is created with: each at the pose and velocities of its read_body_poses() entry (2D poses are
    handed over as an angle, linvel has three entries)."""
    def restored(c, b):
        rot = tuple(b["rotation"]) if dim == 3 else (float(np.arctan2(b["rotation"][1], b["rotation"][0])),)
        return dataclasses.replace(c, translation=tuple(b["translation"]), rotation=rot, linvel=tuple(b["linvel"]) + (0.0,) * (3 - dim),
                                   angvel=tuple(b["angvel"]), com=tuple(b["com"]))
    return [restored(c, b) for c, b in zip(colliders, bodies)]


def _digest(data):
    """the state digest of `data` (wgs_read_diagnostics, WGS_DIAG_DIGEST)"""
    return data.diagnostics(_ffi.DIAG_DIGEST).digest


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if len(a) else 0.0


def grid_of(state):
    """Oracle grid restricted to what matters for parity: (cells, velocity|mass)."""
    cells, mv, dist, aff, closest = state.grid_records()
    return cells, np.asarray(mv, np.float64), dist, aff, closest


def compare_grids(gpu_grid, orc_grid):
    """Both sorted lexicographically by cell; the GPU path may hold the same set of active
    blocks only (bit-exact requirement on cell / block indices)."""
    gc, gv = gpu_grid[0], gpu_grid[1]
    oc, ov = orc_grid[0], orc_grid[1]
    assert gc.shape == oc.shape, f"active node sets differ: {gc.shape} vs {oc.shape}"
    assert np.array_equal(gc, oc), "active node cells differ"
    return gv, ov


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


_MARGINS = []


def report_margin(name, value, bound, **extra):
    """Parity margins are REPORTED, not only bounded: every floating-point comparison appends (measured, bound) to
    $WGS_MARGINS_FILE when it is set (JSON lines; tools/summarize_margins.py reduces such a file to the worst record per check name)."""
    import json
    import os
    rec = dict(test=os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], name=name, value=float(value), bound=float(bound), **extra)
    _MARGINS.append(rec)
    path = os.environ.get("WGS_MARGINS_FILE")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def assert_joined_close(joined, ref, checks, name, ref_order=None, **extra):
    """The joined slabs of a decomposition (sharded.join_slabs) against the single-domain run `ref`, whose particles are in the order
    of the ids (or brought into it by `ref_order`): every id exactly once, then for each (field, tolerance) of `checks` the rel_rms,
    reported under name.format(f=field) with `extra`, below the tolerance."""
    assert joined.exact, joined.problem
    for f, tol in checks:
        want = getattr(ref, f)
        err = rel_rms(joined.fields[f], want if ref_order is None else want[ref_order])
        report_margin(name.format(f=f), err, tol, **extra)
        assert err < tol, (f, err)


def assert_close_to_truth(name, got, ref32, truth, rel_tol, k32=None):
    """fp32 tolerance rule used by every floating-point parity check:
    the HIP result must be within `rel_tol` (relative RMS) of the fp64 oracle. One field has an escape: `affine`
    (C' = APIC matrix minus the stress term) is round-off times E wherever the body moves rigidly — its fp64 value is
    ~0 and a relative bound means nothing —, so there the HIP result may instead be within `k32` = 4 times the error
    the fp32 restatement of the reference's own arithmetic makes against the same fp64 truth (measured: 1.0-2.6 x,
    profiles/r02_parity_margins.json). No other field needs it, and none gets it."""
    if k32 is None:
        k32 = 4.0 if name.startswith("affine") else 0.0
    got = np.asarray(got, np.float64)
    truth = np.asarray(truth, np.float64)
    e_gpu = rms(got - truth)
    e_32 = rms(np.asarray(ref32, np.float64) - truth)
    scale = rms(truth)
    bound = max(rel_tol * scale, k32 * e_32)
    escape = bool(k32 * e_32 > rel_tol * scale)
    if escape and e_gpu > rel_tol * scale:
        # the relative bound means nothing here (truth ~ 0): what is checked, and reported under a name of its own, is the HIP
        # error in multiples of the error the fp32 restatement of the reference's arithmetic makes against the same truth
        report_margin(name + " [escape used: multiples of the fp32 restatement's own error]", e_gpu / e_32, k32, escape_used=True)
    else:
        report_margin(name, e_gpu / scale if scale > 0 else e_gpu, rel_tol, fp32_oracle_err=e_32 / scale if scale > 0 else e_32,
                      escape_available=escape, escape_used=False)
    assert np.isfinite(e_gpu) and e_gpu <= bound, (
        f"{name}: rms err {e_gpu:.3e} > bound {bound:.3e} (scale {scale:.3e}, fp32-oracle err {e_32:.3e})")
    return e_gpu / scale if scale > 0 else e_gpu


def compare_cpic(data, st32, st64, dim, grid_tol, part_tol, min_same=0.995, fields=("pos", "vel", "def_grad", "affine"), h=1.0,
                 truth=None):
    """Parity of a collider (CPIC) scene. `truth` = (dict of fp64 particle arrays, fp64 grid velocity|mass array) may
    replace the fp64 oracle state (golden vectors). Integer results first — active cells, node affinity / sign bits, closest
    collider ids: exact. CPIC has discrete per-particle decisions sitting on fp32 thresholds (sign votes, det M > 1e-8),
    so a few particles may carry other affinity bits than the oracle's; they, and the grid nodes inside their 3^D
    stencil (a node inside a collider can hold 1e-6 of a particle's mass: one such particle moves its velocity by
    O(1)), are left out of the floating-point comparison, and their NUMBER is reported and bounded. Everything else is
    compared against the fp64 oracle with `grid_tol` / `part_tol` (relative RMS)."""
    cells, vm, dist, aff, closest = data.read_grid()
    oc, omv, odist, oaff, oclosest = st32.grid_records()
    assert np.array_equal(cells, oc), "active node cells differ"
    assert np.array_equal(aff, oaff), "node affinity / sign bits differ"
    assert np.array_equal(closest, oclosest), "closest collider ids differ"
    got = data.read_particles()
    same = got.cdf_affinity == st32.arr["cdf_affinity"]
    report_margin("particle affinity mismatch fraction", 1.0 - float(same.mean()), 1.0 - min_same, count=int((~same).sum()))
    assert same.mean() >= min_same, f"affinity bits agree for only {same.mean():.5f} of the particles"
    keep = np.ones(len(cells), bool)
    if not same.all():
        h = np.float32(h)
        bad = []
        for pos in (st32.arr["pos"][~same], got.pos[~same]):          # stencils at either position (they agree to 1e-6)
            base = (np.rint(pos.astype(np.float32) / h) - 1).astype(np.int64)
            for off in np.ndindex(*([3] * dim)):
                bad.append(base + np.array(off))
        bad = np.unique(np.concatenate(bad), axis=0)
        key = lambda c: (c[:, 0] * 4099 + c[:, 1]) * 4099 + (c[:, 2] if dim == 3 else 0)
        keep = ~np.isin(key(cells.astype(np.int64)), key(bad))
        report_margin("grid nodes left out (stencils of mismatching particles)", float((~keep).mean()), 0.02, count=int((~keep).sum()))
        assert (~keep).mean() < 0.02
    t_arr, o64 = truth if truth is not None else (st64.arr, grid_of(st64)[1])
    assert_close_to_truth("grid velocity (CPIC)", vm[keep][:, :dim], omv[keep][:, :dim], o64[keep][:, :dim], grid_tol)
    assert_close_to_truth("grid mass (CPIC)", vm[keep][:, dim], omv[keep][:, dim], o64[keep][:, dim], grid_tol)
    for f in fields:
        assert_close_to_truth(f + " (CPIC)", getattr(got, f)[same], st32.arr[f][same], t_arr[f][same], part_tol)
    return got, same
