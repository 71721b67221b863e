"""-m gpu: force fields (wgs_set_force_fields) against the rule of tests/force_truth.py (validated on the CPU by
tests/test_force_truth.py, which also shows from the truth alone that no node of these scenes lies within rounding of a region face).

The walls' method. Twin runs of one upload without and with fields: the first P2G does not depend on the fields, so the forced grid
must be the rule applied to the twin's grid, node by node within force_truth.node_bound — every node outside the region and every
massless node bit for bit the twin's, every mass bit for bit. The particles of that substep against the fp64 truth substep with
fields, end to end and from the kernel's own forced grid (the check that fails when only Dev::nodes is rewritten: the fused G2P stages
its tiles from the slabs). With walls, with a floor collider, a model table and Drucker-Prager particles; determinism; neutrality;
refusals; the momentum a uniform field adds, a drag that prescribes the velocity, a planetoid that stays together.

The scenes are force_truth's: region faces between a block's last node and the next block's first, in the middle of a block, at a
negative coordinate, and a ball whose bounding box reaches a block the ball does not."""
import ctypes as C
import functools

import numpy as np
import pytest

import cpic_truth as CP
import force_truth as FT
import transfer_truth as T
import wall_truth as W
from gpu_common import _start
from helpers import _digest, debug, new_data, pipeline, report_margin
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import (FORCE_NONE, WALL_SEPARATE, WALL_SLIP, WALL_STICKY, DruckerPrager, ForceField, ParticlePhase, Wall)
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider, SimulationParams

pytestmark = pytest.mark.gpu
H_OF = {2: (1.0, 0.3), 3: (0.3, 1.0)}       # the two cell widths of force_truth.CASES per dimension, alternating over the cases


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(sc, nsteps=1, **kw):
    _, data = new_data(sc, **kw)
    pipeline(sc["particles"].dim).step(data, nsteps)
    data.sync()
    return data


@functools.lru_cache(maxsize=None)
def _twin(d, h, seed=0):
    """the cloud of (d, h) and the grid one substep WITHOUT fields leaves: computed once, shared, never changed"""
    sc = FT.cloud(d, h, seed)
    cells, vm = _run(sc).read_grid()[:2]
    cells.setflags(write=False)
    vm.setflags(write=False)
    return sc, cells, vm


def _check_nodes(tag, d, h, dt, fields, c0, vm0, c1, vm1, fails, walls=None, moved_min=50):
    """the forced grid (c1, vm1) against the rule applied to the twin's grid (c0, vm0): bounds, bits, masses; returns the member mask"""
    assert np.array_equal(c0, c1), f"{tag}: the fields changed the active cells"
    assert FT.ambiguous(c0, h, fields).sum() == 0
    v0, m0 = vm0[:, :d], vm0[:, d]
    want = FT.apply(c0, v0, m0, h, dt, fields)
    bound = FT.node_bound(c0, v0, m0, h, dt, fields)
    if walls is not None:
        bound = W.node_bound(c0, want, walls, bound)
        want = W.apply(c0, want, walls)
    err = np.linalg.norm(vm1[:, :d].astype(np.float64) - want, axis=1)
    hit = FT.members(c0, h, fields).any(1) & (m0 > 0)
    T.check(f"{tag}: forced node velocity", err, bound, fails, sel=hit)
    assert np.array_equal(_u32(vm1[:, d]), _u32(m0)), f"{tag}: a field touched a node's mass"
    if walls is None:
        same = np.array_equal(_u32(vm1[~hit, :d]), _u32(v0[~hit]))
        assert same, f"{tag}: a node outside every region, or without mass, is not the twin's bit for bit"
    moved = hit & (np.linalg.norm(want - v0.astype(np.float64), axis=1) > 100.0 * np.maximum(bound, 1e-300))
    assert moved.sum() > moved_min, f"{tag}: the fields change only {int(moved.sum())} nodes of this scene by more than 100 bounds"
    return hit


# ------------------------------------------------------------------------------------------------ 1. node by node
NODE_CASES = [(d, k, p, reg, H_OF[d][(i + j) % 2]) for d in (2, 3) for i, (k, p) in enumerate(FT.KINDS) for j, reg in enumerate(FT.REGIONS)]


@pytest.mark.parametrize("d,kind,p,region,h", NODE_CASES)
def test_node_by_node(hip_libs, d, kind, p, region, h):
    sc, c0, vm0 = _twin(d, h)
    fields = [FT.field(kind, p, d, h, region)]
    c1, vm1 = _run(sc, forces=fields).read_grid()[:2]
    fails = []
    tag = f"forces {d}D h={h} {kind}{p} {region}"
    hit = _check_nodes(tag, d, h, sc["params"].dt, fields, c0, vm0, c1, vm1, fails)
    assert (vm0[:, d] == 0).sum() > 20, "the scene has no massless node"
    if region != "all":
        assert (~hit & (vm0[:, d] > 0)).sum() > 20, "the scene has no massy node outside the region"
        n_in, n_out, n_cut, corner = FT.block_classes(c0, h, fields[0], d)
        assert n_in > 0 and n_out > 0 and n_cut > 0 and (corner > 0) == (region == "ball"), (n_in, n_out, n_cut, corner)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 2. array order and the maximum
@pytest.mark.parametrize("d,h", FT.CASES)
def test_array_order_and_eight_fields(hip_libs, d, h):
    sc, c0, vm0 = _twin(d, h)
    dt = sc["params"].dt
    drag, uni = FT.field("drag", 0, d, h, "box"), FT.field("uniform", 0, d, h, "all")
    fails, got = [], {}
    for name, fields in (("drag then uniform", [drag, uni]), ("uniform then drag", [uni, drag]), ("eight", FT.eight(d, h))):
        data = _run(sc, forces=fields)
        c1, vm1 = data.read_grid()[:2]
        _check_nodes(f"forces {d}D h={h} {name}", d, h, dt, fields, c0, vm0, c1, vm1, fails)
        got[name] = vm1[:, :d].astype(np.float64)
        back = data.force_fields()
        assert len(back) == len(fields) and [f.kind for f in back] == [FORCE_NONE if f is None else f.kind for f in fields]
    both = FT.members(c0, h, [drag]).any(1) & (vm0[:, d] > 0)
    b = FT.node_bound(c0, vm0[:, :d], vm0[:, d], h, dt, [drag, uni]) + FT.node_bound(c0, vm0[:, :d], vm0[:, d], h, dt, [uni, drag])
    apart = np.linalg.norm(got["drag then uniform"] - got["uniform then drag"], axis=1)
    assert both.sum() > 50 and np.all(apart[both] > 100.0 * b[both]), "the two orders are not told apart on the nodes both fields hold"
    assert np.array_equal(got["drag then uniform"][~both], got["uniform then drag"][~both])
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 3. particle by particle
def _mixed(d, h):
    return [FT.field("uniform", 0, d, h, "box"), FT.field("radial", 1, d, h, "all"), FT.field("vortex", 2, d, h, "ball"), FT.field("drag", 0, d, h, "box")]


def _gathered_from_all_sources(ps, h, d, node_cells):
    """how many blocks that hold one of `node_cells` have all 2^D "-" neighbour blocks bearing particles"""
    have = set(map(tuple, np.unique(T.assoc_cell(ps.pos, h) // T.bw_of(d), axis=0).tolist()))
    blocks = np.unique(node_cells // T.bw_of(d), axis=0)
    return sum(all(tuple(np.array(b) - np.array(o)) in have for o in np.ndindex(*([2] * d))) for b in map(tuple, blocks.tolist()))


@pytest.mark.parametrize("d,h", FT.CASES)
def test_first_substep_particle_by_particle(hip_libs, d, h):
    """Fails when k_grid_forces rewrites Dev::nodes alone: the fused G2P stages its velocity tiles from the slabs."""
    sc = FT.cloud(d, h, seed=2)
    ps, dt = sc["particles"], sc["params"].dt
    fields = _mixed(d, h)
    data = _run(sc, forces=fields)
    cells, vm = data.read_grid()[:2]
    got = data.read_particles()
    inp = T.Inputs.of(ps)
    st, gr, vf, bnd, pt = FT.substep(inp, h, dt, T.GRAVITY[:d], fields)
    fails = []
    i = gr.lookup(cells)
    hit = i >= 0
    assert hit.sum() == len(gr.keys)
    assert np.array_equal(vm[hit, d] > 0, gr.mass[i[hit]] > 0), "truth and kernel disagree on which nodes have mass"
    T.check(f"forces {d}D h={h}: forced node velocity end to end", np.linalg.norm(vm[hit, :d].astype(np.float64) - vf[i[hit]], axis=1), bnd[i[hit]], fails)
    T.check_particles(f"forces {d}D h={h} end to end", pt, got, sc["model"], fails)
    iso = T.isolated(inp, st, cells, vm[:, :d], dt)
    T.check_particles(f"forces {d}D h={h} isolated G2P", iso, got, sc["model"], fails)
    # the scene does test it: the fields change what many particles gather, and forced nodes are held by all 2^D source slabs
    m = FT.members(gr.cells, h, fields).any(1) & (gr.mass > 0)
    _, _, pt0 = T.substep(inp, h, dt, T.GRAVITY[:d])
    moved = np.linalg.norm(pt.vel - pt0.vel, axis=1) > 10.0 * (pt.b_vel + pt0.b_vel)
    assert m[gr.inv].any(1).sum() > ps.n // 4 and moved.sum() > ps.n // 10, (int(m[gr.inv].any(1).sum()), int(moved.sum()))
    assert _gathered_from_all_sources(ps, h, d, gr.cells[m]) > 0, "no forced node is gathered from all 2^D source slabs"
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 4. with walls
WALL_PLANES = {3: [(-4, 9), (-3, 8), (-5, 10)], 2: [(-5, 17), (-6, 20)]}
WALL_TYPES = {3: [WALL_STICKY, WALL_SLIP, WALL_SLIP, WALL_SEPARATE, WALL_SEPARATE, WALL_STICKY], 2: [WALL_SEPARATE, WALL_STICKY, WALL_SLIP, WALL_SEPARATE]}


def _walls(d):
    return [Wall(WALL_TYPES[d][f], 0.0, WALL_PLANES[d][f >> 1][f & 1]) for f in range(2 * d)]


def _pushes(d, h):
    """UNIFORM fields that push into every face: outward from the middle of the box of walls, one field per half-space"""
    out = []
    for k in range(d):
        lo, hi = WALL_PLANES[d][k]
        mid = (0.5 * (lo + hi) + 0.5) // 1 + 0.5
        for side, c in ((-1.0, (lo - 40 + mid) / 2.0), (1.0, (hi + 40 + mid) / 2.0)):
            a = [0.0] * d
            a[k] = side * 600.0 * h
            centre, half = [0.0] * d, [1000.0 * h] * d
            centre[k], half[k] = c * h, abs(c - mid) * h
            out.append(ForceField.uniform(tuple(a)).within_box(tuple(centre), tuple(half)))
    return out


@pytest.mark.parametrize("d,h", FT.CASES)
def test_fields_run_in_front_of_the_walls(hip_libs, d, h):
    sc, c0, vm0 = _twin(d, h)
    walls, fields = _walls(d), _pushes(d, h)
    data = _run(sc, forces=fields, walls=walls)
    c1, vm1 = data.read_grid()[:2]
    fails = []
    _check_nodes(f"forces and walls {d}D h={h}", d, h, sc["params"].dt, fields, c0, vm0, c1, vm1, fails, walls=walls)
    assert not fails, "\n".join(fails)
    # the pushes do drive the wall nodes into the faces: without the walls they move into them
    pushed = FT.apply(c0, vm0[:, :d], vm0[:, d], h, sc["params"].dt, fields)
    m = W.members(c0, walls)
    for f in range(2 * d):
        into = pushed[m[:, f], f >> 1] * (1.0 if f & 1 else -1.0) > 0
        assert into.sum() > 10, f
    done = 1
    for upto in (1, 2, 50):
        if upto > done:
            pipeline(d).step(data, upto - done)
            data.sync()
        done = upto
        cells, vm = data.read_grid()[:2]
        m = W.members(cells, walls)
        assert np.all(np.isfinite(vm))
        for f, w in enumerate(walls):
            k, sel = f >> 1, m[:, f]
            assert sel.any(), (upto, f)
            if w.type == WALL_STICKY:
                assert not vm[sel, :d].any(), f"substep {upto}: a sticky node of face {f} moves"
            elif w.type == WALL_SLIP:
                assert not vm[sel, k].any(), f"substep {upto}: a slip node of face {f} has a normal velocity"
            else:
                assert np.all(vm[sel, k] <= 0.0 if f & 1 else vm[sel, k] >= 0.0), f"substep {upto}: a separating node of face {f} moves into the wall"


# ------------------------------------------------------------------------------------------------ 5. with other features
def _xv(tag, iso, got, fails):
    """x and v of every particle from the kernel's own forced grid (F and C' are the model's: their own files judge them)"""
    T.check(f"{tag}: x", np.linalg.norm(got.pos.astype(np.float64) - iso.x, axis=1), iso.b_x, fails)
    T.check(f"{tag}: v", np.linalg.norm(got.vel.astype(np.float64) - iso.vel, axis=1), iso.b_vel, fails)


@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
def test_with_a_floor_collider(hip_libs, monkeypatch, d, h):
    """the CPIC shapes (the two-launch form of the fused G2P as well): the nodes by twins, the particles from the kernel's own forced
    grid and its own CPIC decisions (cpic_truth)"""
    sc = FT.cloud(d, h, seed=5)
    half, centre = [1000.0 * h] * d, [0.0] * d
    half[1], centre[1] = 2.0 * h, (FT.EXTENT[d][0] + 4.0) * h
    sc["colliders"] = [Collider.cuboid(tuple(half), tuple(centre), **({"rotation": (0.0,)} if d == 2 else {}))]
    ps, prm, fields = sc["particles"], sc["params"], _mixed(d, h)
    c0, vm0 = _run(sc).read_grid()[:2]
    for two in (False, True):
        with debug(monkeypatch, *(["G2P_TWO_LAUNCHES"] if two else [])):
            _, data = new_data(sc, forces=fields)
            poses = data.read_body_poses()
            pipeline(d).step(data, 1)
            data.sync()
        cells, vm, _, aff, closest = data.read_grid()
        got = data.read_particles()
        fails = []
        tag = f"forces with a floor {d}D h={h} two_launches={two}"
        _check_nodes(tag, d, h, prm.dt, fields, c0, vm0, cells, vm, fails)
        f = CP.Fields(got.cdf_affinity, got.cdf_normal.astype(np.float64), got.cdf_dist.astype(np.float64), cells, aff, closest)
        iso = CP.substep(T.Inputs.of(ps), h, prm.dt, prm.gravity, f, CP.Motion.of(sc["colliders"], d, poses), own_grid=(cells, vm[:, :d]))
        CP.check_result(f"{tag} isolated G2P", iso, None, None, got, sc["model"], fails)
        assert (got.cdf_affinity != 0).sum() > 0.02 * ps.n, "the floor is not felt by the cloud"
        assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d,h", [(2, 1.0), (3, 0.3)])
def test_with_a_model_table(hip_libs, d, h):
    sc = FT.cloud(d, h, seed=6)
    table = (np.arange(sc["particles"].n) % 2).astype(np.uint8)          # corotated and neo-Hookean particles side by side
    fields = _mixed(d, h)
    c0, vm0 = _run(sc, models=table).read_grid()[:2]
    data = _run(sc, models=table, forces=fields)
    cells, vm = data.read_grid()[:2]
    fails = []
    _check_nodes(f"forces with a model table {d}D h={h}", d, h, sc["params"].dt, fields, c0, vm0, cells, vm, fails)
    inp = T.Inputs.of(sc["particles"])
    _xv(f"forces with a model table {d}D h={h} isolated G2P", T.isolated(inp, T.Stencil(inp, h), cells, vm[:, :d], sc["params"].dt), data.read_particles(), fails)
    assert np.array_equal(data.read_particle_models(), table)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
def test_with_drucker_prager_particles(hip_libs, d, h):
    ps = scenes.random_cloud(3000 if d == 2 else 6000, dim=d, seed=40 + d, extent=12.0 * h, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25), phase=None,
                             vel_scale=3.0 * h, perturb_F=0.02, perturb_C=0.2)
    sc = dict(particles=ps, params=SimulationParams(gravity=T.GRAVITY[:d], dt=T.DT), colliders=[], cell_width=h, grid_capacity=4096, model=0)
    fields = _mixed(d, h)
    runs = []
    for f in (None, fields):
        pipe, data = _start(sc, forces=f)
        pipe.step(data, 1)
        data.sync()
        runs.append(data)
    (c0, vm0), (cells, vm) = runs[0].read_grid()[:2], runs[1].read_grid()[:2]
    fails = []
    _check_nodes(f"forces with Drucker-Prager {d}D h={h}", d, h, T.DT, fields, c0, vm0, cells, vm, fails)
    inp = T.Inputs.of(ps)
    got = runs[1].read_particles()
    _xv(f"forces with Drucker-Prager {d}D h={h} isolated G2P", T.isolated(inp, T.Stencil(inp, h), cells, vm[:, :d], T.DT), got, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
def test_same_bits(hip_libs, monkeypatch, d, h):
    sc = FT.cloud(d, h, seed=7, n=4000 if d == 3 else 2000)
    fields = FT.eight(d, h)
    a, b = _run(sc, 20, forces=fields), _run(sc, 20, forces=fields)
    assert _digest(a) == _digest(b)
    ga, gb = a.read_grid()[:2], b.read_grid()[:2]
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(_u32(ga[1]), _u32(gb[1]))
    with debug(monkeypatch, "GU_OWN_LAUNCH"):
        c = _run(sc, 20, forces=fields)
    assert _digest(c) == _digest(a), "the fields differ behind the grid update as a launch of its own"
    gc = c.read_grid()[:2]
    assert np.array_equal(ga[0], gc[0]) and np.array_equal(_u32(ga[1]), _u32(gc[1]))
    assert _digest(_run(sc, 20)) != _digest(a)


# ------------------------------------------------------------------------------------------------ 7. neutrality
@pytest.mark.parametrize("d,h", [(2, 1.0), (3, 0.3)])
def test_fields_that_do_nothing_change_no_bit(hip_libs, d, h):
    sc = FT.cloud(d, h, seed=8, n=4000 if d == 3 else 2000)
    never = _digest(_run(sc, 20))
    _, data = new_data(sc, forces=FT.eight(d, h))
    data.set_force_fields(None)
    assert data.force_fields() == []
    pipeline(d).step(data, 20)
    data.sync()
    assert _digest(data) == never, "fields set and removed"
    c = tuple(np.array(FT.CENTER[d]) * h)
    idle = [ForceField.uniform((0.0,) * d), ForceField.radial(c, 0.0, 2, h), ForceField.vortex(c, 0.0, FT.AXIS, 1, h), ForceField.drag(0.0, (3.0,) * d),
            None, ForceField()]
    assert _digest(_run(sc, 20, forces=idle)) == never, "fields of strength 0 and rate 0"
    nowhere = [FT.field(k, p, d, h).within_box((-500.0 * h,) * d, (3.5 * h,) * d) for k, p in (("uniform", 0), ("radial", 3), ("drag", 0))] + \
              [FT.field("vortex", 1, d, h).within_ball((900.0 * h,) * d, 20.0 * h)]
    assert _digest(_run(sc, 20, forces=nowhere)) == never, "regions that hold no node"
    before = _run(sc, 2).stats()["device_bytes"]
    assert _run(sc, 2, forces=FT.eight(d, h)).stats()["device_bytes"] == before, "the fields take device memory"


# ------------------------------------------------------------------------------------------------ 8. refusals and getters
@pytest.mark.parametrize("d", [2, 3])
def test_refusals_change_nothing(hip_libs, d):
    h = 1.0
    sc = FT.cloud(d, h, seed=9, n=2000)
    good = [FT.field("radial", 2, d, h, "ball"), None, FT.field("drag", 0, d, h, "box"), FT.field("vortex", 1, d, h, "all")]
    pipe, data = new_data(sc, forces=good)
    pipe.step(data, 2)
    data.sync()
    ref = new_data(sc, forces=good)[1]
    pipe.step(ref, 3)
    ref.sync()
    lib, hd = data.lib, data._h
    answered = data.force_fields()
    assert len(answered) == 4 and answered[1].kind == FORCE_NONE and answered[0].falloff == 2 and answered[2].region == good[2].region

    def raw(n=1, **kw):
        a = (_ffi.ForceField * 9)()
        a[0].kind, a[0].softening, a[0].vec[:] = 2, 1.0, [0.0, 1.0, 0.0]
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                getattr(a[0], k)[:] = list(v)
            else:
                setattr(a[0], k, v)
        return a, n

    nan, inf = float("nan"), float("inf")
    bad = [raw(9), raw(kind=5), raw(kind=0xffffffff), raw(falloff=4), raw(region=3), raw(strength=nan), raw(softening=inf), raw(center=[0.0, nan, 0.0]),
           raw(vec=[inf, 0.0, 0.0]), raw(region_center=[nan, 0.0, 0.0]), raw(region_half=[0.0, 0.0, nan]), raw(softening=-1.0),
           raw(kind=2, falloff=1, softening=0.0), raw(kind=3, falloff=3, softening=0.0), raw(kind=4, strength=-1.0),
           raw(region=1, region_half=[1.0, -1.0, 1.0]), raw(region=2, region_half=[-1.0, 0.0, 0.0])]
    if d == 3:
        bad += [raw(kind=3, vec=[0.0, 0.0, 0.0]), raw(region=1, region_half=[1.0, 1.0, -1.0])]
    invalid, unsupported = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    for a, n in bad:
        assert lib.wgs_set_force_fields(hd, a, n) == invalid and lib.wgs_last_error(), bytes(a)[:68]
        assert data.force_fields() == answered
    n = C.c_uint32(77)
    out = (_ffi.ForceField * 8)()
    assert lib.wgs_set_force_fields(hd, None, 1) == invalid and lib.wgs_set_force_fields(None, raw()[0], 1) == invalid
    assert lib.wgs_get_force_fields(hd, None, C.byref(n)) == invalid and lib.wgs_get_force_fields(hd, out, None) == invalid
    assert lib.wgs_get_force_fields(None, out, C.byref(n)) == invalid and n.value == 77
    # what a refusal must not reject: the third components of a 2D field's region, a zero axis in 2D, softening 0 at falloff 0
    if d == 2:
        assert lib.wgs_set_force_fields(hd, *raw(kind=3, vec=[0.0, 0.0, 0.0])) == _ffi.WGS_OK
        assert lib.wgs_set_force_fields(hd, *raw(region=1, region_half=[1.0, 1.0, -1.0])) == _ffi.WGS_OK
    assert lib.wgs_set_force_fields(hd, *raw(kind=2, falloff=0, softening=0.0)) == _ffi.WGS_OK
    assert lib.wgs_set_force_fields(hd, *raw(kind=0, strength=nan)) == _ffi.WGS_OK, "a NONE entry's floats are not read"
    data.set_force_fields(good)
    assert data.force_fields() == answered
    pipe.step(data, 1)
    data.sync()
    assert _digest(data) == _digest(ref), "the refusals left a trace in the next substep"
    shards, _ = lockstep_slabs(pipe, sc, 2)
    for s in shards:
        C.memset(out, 0x5a, C.sizeof(out))
        assert lib.wgs_set_force_fields(s._h, *raw()) == unsupported and b"single-domain data only" in lib.wgs_last_error()
        assert lib.wgs_get_force_fields(s._h, out, C.byref(n)) == unsupported and bytes(out) == b"\x5a" * C.sizeof(out) and n.value == 77


# ------------------------------------------------------------------------------------------------ 9. physics in the small
@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
def test_a_uniform_field_adds_M_a_dt_to_the_grid_momentum(hip_libs, d, h):
    """The fixed-point sums are exact sums of rounded terms: each differs from the sum of its fp64 terms by at most N 2^(exponent - 1),
    N = 64 x active blocks (the header's bound); the rule itself by sum m_i bound_i."""
    sc, c0, vm0 = _twin(d, h)
    a = FT.field("uniform", 0, d, h)
    dt = sc["params"].dt
    s0 = _run(sc).diagnostics(_ffi.DIAG_GRID).sums
    s1 = _run(sc, forces=[a]).diagnostics(_ffi.DIAG_GRID).sums
    mass = vm0[:, d].astype(np.float64)
    want = mass.sum() * float(np.float32(dt)) * np.asarray(FT.Field(a, d).vec)
    rule = (mass * FT.node_bound(c0, vm0[:, :d], vm0[:, d], h, dt, [a])).sum()
    own = len(c0) * (2.0 ** (s0["grid_momentum"].exponent - 1) + 2.0 ** (s1["grid_momentum"].exponent - 1))
    err = np.abs(s1["grid_momentum"].value - s0["grid_momentum"].value - want).max()
    report_margin(f"forces {d}D h={h}: grid momentum added by a uniform field against M a dt", float(err), float(own + rule))
    assert err <= own + rule and np.abs(want).min() > 1000.0 * (own + rule)
    assert np.array_equal(s1["grid_mass"].fixed, s0["grid_mass"].fixed)


@pytest.mark.parametrize("d,h", [(2, 1.0), (3, 0.3)])
def test_a_huge_drag_prescribes_the_velocity(hip_libs, d, h):
    sc = FT.cloud(d, h, seed=10, n=4000 if d == 3 else 2000)
    u = np.array([4.0, -3.0, 2.5][:d], np.float32) * np.float32(h)
    fields = [ForceField.drag(1e12, tuple(float(x) for x in u))]
    _, data = new_data(sc, forces=fields)
    pipeline(d).step(data, 1)
    data.sync()
    cells, vm = data.read_grid()[:2]
    massy = vm[:, d] > 0
    err = np.linalg.norm(vm[massy, :d].astype(np.float64) - u.astype(np.float64), axis=1)
    report_margin(f"forces {d}D h={h}: drag at 1e12 / s, node velocity against the target (2 u |u|)", float(err.max()), 2.0 * T.U32 * float(np.linalg.norm(u)))
    assert massy.sum() > 100 and np.all(err <= 2.0 * T.U32 * np.linalg.norm(u))
    assert not vm[~massy, :d].any()
    # every particle after 20 substeps: the truth substep from the state before the last one
    pipeline(d).step(data, 18)
    data.sync()
    before = data.read_particles()
    pipeline(d).step(data, 1)
    data.sync()
    got = data.read_particles()
    _, _, _, _, pt = FT.substep(T.Inputs.of(before), h, sc["params"].dt, T.GRAVITY[:d], fields)
    fails = []
    T.check(f"forces {d}D h={h}: drag at 1e12 / s, particle velocity after 20 substeps", np.linalg.norm(got.vel.astype(np.float64) - pt.vel, axis=1), pt.b_vel, fails)
    assert not fails, "\n".join(fails)
    assert np.abs(got.vel.astype(np.float64) - u).max() < 1e-4 * np.linalg.norm(u)


@pytest.mark.parametrize("d", [2, 3])
def test_a_vortex_tank_spins_up_between_its_walls(hip_libs, d):
    """scenes.vortex_tank: Tait fluid between grid walls, a VORTEX and a DRAG zone. The fluid gains angular momentum about the vortex's
    axis (its twin without fields has none to speak of), stays finite and stays between the walls."""
    sc = scenes.vortex_tank(d, tank=(16, 8, 16))
    ps, h = sc["particles"], sc["cell_width"]
    mid = np.array(sc["forces"][0].center[:d], np.float64)

    def spin(data):
        got = data.read_particles()
        for name in ("pos", "vel", "def_grad", "affine"):
            assert np.all(np.isfinite(getattr(got, name))), name
        r, v, m = got.pos.astype(np.float64) - mid, got.vel.astype(np.float64), got.mass.astype(np.float64)
        about = r[:, 0] * v[:, 1] - r[:, 1] * v[:, 0] if d == 2 else r[:, 2] * v[:, 0] - r[:, 0] * v[:, 2]
        return float((m * about).sum()), float((m * np.linalg.norm(r, axis=1) * np.linalg.norm(v, axis=1)).sum()), got

    with_fields, scale, got = spin(_run(sc, 40))
    without, _, _ = spin(_run(sc, 40, forces=None))
    assert [f.kind for f in new_data(sc)[1].force_fields()] == [f.kind for f in sc["forces"]]
    assert with_fields > 0.2 * scale and with_fields > 20.0 * abs(without), (with_fields, scale, without)
    for k in ((0,) if d == 2 else (0, 2)):
        lo, hi = sc["walls"][2 * k], sc["walls"][2 * k + 1]
        assert got.pos[:, k].min() >= (lo.plane - 1.5) * h - 1e-3 * h and got.pos[:, k].max() <= (hi.plane + 1.5) * h + 1e-3 * h
    assert got.pos[:, 1].min() >= (sc["walls"][2].plane - 1.5) * h - 1e-3 * h


@pytest.mark.parametrize("d", [2, 3])
def test_a_planetoid_stays_together_and_its_control_does_not(hip_libs, d):
    radius = 4.0 if d == 3 else 6.0
    far = {}
    for with_field in (True, False):
        sc = scenes.planetoid(d, radius=radius, with_field=with_field)
        _, data = new_data(sc)
        assert len(data.force_fields()) == (1 if with_field else 0)
        for _ in range(4):
            pipeline(d).step(data, 50)
            data.sync()
        pos = data.read_positions().astype(np.float64)
        assert np.all(np.isfinite(pos))
        far[with_field] = np.linalg.norm(pos - sc["centre"], axis=1).max() / sc["start_radius"]
    report_margin(f"planetoid {d}D: furthest particle after 200 substeps (start radii)", float(far[True]), 2.0, control=float(far[False]))
    assert far[True] <= 2.0, f"a particle of the planetoid is {far[True]:.2f} start radii from the centre"
    assert far[False] > 2.0, f"the control without the field stays within {far[False]:.2f} start radii: the scene tests nothing"
