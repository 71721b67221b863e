"""-m gpu: domain walls (wgs_set_domain_walls) against the rule of tests/wall_truth.py (validated on the CPU by
tests/test_wall_truth.py).

Twin runs of one upload with and without walls: the first P2G does not depend on the walls, so the walled grid must be the numpy
rule applied to the twin's grid — bit for bit where friction == 0, within 8 u |v| where not. The particles of that substep against
the fp64 truth substep with walls, end to end and from the kernel's own walled grid (the check that fails when the slab copies the
fused G2P stages are not rewritten). Postconditions after 1, 2 and 50 substeps; containment of a cloud thrown at every face; the
same bits for either form of the grid update; refusals; a tank of domain walls.

The planes are chosen so that the kernel's wave-uniform reject can go wrong in every way it can: a plane in the middle of a block, on
a block's first and on its last node (3D: 4 and 7, 2D: 8 and 15), a negative plane, blocks wholly inside a face, and nodes in two
and three faces (the cloud covers the corners)."""
import ctypes as C

import numpy as np
import pytest

import transfer_truth as T
import wall_truth as W
from helpers import _digest, debug, new_data, pipeline, report_margin
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import WALL_NONE, WALL_SEPARATE, WALL_SLIP, WALL_STICKY, Wall
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider

pytestmark = pytest.mark.gpu

# planes (low, high) per axis; A: first / last node of a block, negative, middle; B: last node as a LOW plane, first node as a HIGH one
PLANES = {
    (3, "A"): [(4, 11), (-3, 7), (5, 8)],
    (3, "B"): [(7, 12), (5, 9), (-3, 4)],
    (2, "A"): [(8, 15), (-3, 5)],
    (2, "B"): [(5, 16), (15, 24)],
}
CASES = [(2, 1.0, "A"), (2, 0.3, "B"), (3, 0.3, "A"), (3, 1.0, "B")]
TYPES = {"sticky": WALL_STICKY, "slip": WALL_SLIP, "separate": WALL_SEPARATE}


def _walls(d, which, types, friction=0.0, friction_axis=None):
    """2 d faces at PLANES[d, which]; `types`: one type, or one per face; friction on the faces of `friction_axis` only (so that no
    node lies in two frictional faces: the 8 u |v| of one face is then the whole rounding bound)"""
    out = []
    for f in range(2 * d):
        k = f >> 1
        t = types if isinstance(types, int) else types[f]
        fr = friction if (friction_axis is None or friction_axis == k) and t != WALL_STICKY else 0.0
        out.append(Wall(t, fr, PLANES[d, which][k][f & 1]))
    return out


MIXED = {3: [WALL_STICKY, WALL_SLIP, WALL_SLIP, WALL_SEPARATE, WALL_SEPARATE, WALL_SLIP], 2: [WALL_SEPARATE, WALL_STICKY, WALL_SLIP, WALL_SEPARATE]}


def _cloud(d, h, which, seed=0, floor=False, n=None):
    """a cloud over every plane of PLANES[d, which] and two cells beyond: particles in the "-" neighbour blocks of every wall node,
    blocks wholly inside the low faces, every edge and corner"""
    rng = np.random.default_rng(100 * d + seed)
    lo = min(p[0] for p in PLANES[d, which]) - 6
    hi = max(p[1] for p in PLANES[d, which]) + 4
    n = n or (9000 if d == 3 else 3000)
    sc = T._finish(rng.uniform(lo * h, hi * h, (n, d)), h, rng, vel_scale=6.0 * h)
    if floor:   # a fixed floor cuboid under the cloud's lower third as well: the CPIC paths read what the walls wrote
        half = [1000.0 * h] * d
        half[1] = 2.0 * h
        centre = [0.0] * d
        centre[1] = (lo + 4.0) * h
        sc["colliders"] = [Collider.cuboid(tuple(half), tuple(centre), **({"rotation": (0.0,)} if d == 2 else {}))]
    return sc


def _twins(sc, walls, nsteps=1):
    """the same upload without and with `walls`, `nsteps` substeps each: (data0, data1)"""
    out = []
    for w in (None, walls):
        _, data = new_data(sc, walls=w)
        pipeline(sc["particles"].dim).step(data, nsteps)
        data.sync()
        out.append(data)
    return out


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _blocks_wholly_inside(cells, m, d):
    """how many (block, face) pairs have all 64 nodes of the block inside the face"""
    _, inv = np.unique(T.node_key(cells // T.bw_of(d)), return_inverse=True)
    return sum(int((np.bincount(inv.reshape(-1), m[:, f].astype(np.float64)) == 64).sum()) for f in range(m.shape[1]))


# ------------------------------------------------------------------------------------------------ 1. node by node
@pytest.mark.parametrize("d,h,which", CASES)
@pytest.mark.parametrize("typ", list(TYPES))
def test_frictionless_walls_node_by_node_bit_for_bit(hip_libs, d, h, which, typ):
    sc = _cloud(d, h, which)
    walls = _walls(d, which, TYPES[typ])
    d0, d1 = _twins(sc, walls)
    (c0, vm0), (c1, vm1) = d0.read_grid()[:2], d1.read_grid()[:2]
    assert np.array_equal(c0, c1)
    want = W.apply(c0, vm0[:, :d], walls)
    m = W.members(c0, walls)
    assert m.sum(1).max() == d and (m.sum(1) == 2).any(), "the cloud reaches no node in two / three faces"
    assert _blocks_wholly_inside(c0, m, d) > 0, "no block of the scene lies wholly inside a face"
    assert (W.bits(want) != _u32(vm0[:, :d])).any(), "the walls change no node of this scene"
    bad = np.nonzero((W.bits(want) != _u32(vm1[:, :d])).any(1))[0]
    assert not len(bad), f"{len(bad)} nodes differ from the rule, first at cell {c0[bad[0]].tolist()}: {vm1[bad[0], :d]} want {want[bad[0]]} from {vm0[bad[0], :d]}"
    assert np.array_equal(_u32(vm1[:, d]), _u32(vm0[:, d])), "a wall touched a node's mass"


@pytest.mark.parametrize("d,h,which,floor", [c + (False,) for c in CASES] + [(3, 0.3, "A", True), (2, 0.3, "B", True)])
def test_walls_with_friction_node_by_node(hip_libs, d, h, which, floor):
    """floor: once per dimension in a scene that has a floor collider as well"""
    sc = _cloud(d, h, which, seed=1, floor=floor)
    walls = _walls(d, which, MIXED[d], friction=0.4, friction_axis=1 if d == 3 else 0)
    d0, d1 = _twins(sc, walls)
    (c0, vm0), (c1, vm1) = d0.read_grid()[:2], d1.read_grid()[:2]
    assert np.array_equal(c0, c1)
    v0 = vm0[:, :d].astype(np.float64)
    want = W.apply(c0, v0, walls)
    L, nf = W.lipschitz(c0, walls)
    assert nf.max() == 1 and (nf == 1).sum() > 50
    err = np.linalg.norm(vm1[:, :d].astype(np.float64) - want, axis=1)
    bound = W.C_WALL * T.U32 * np.linalg.norm(v0, axis=1)
    fr = nf == 1
    worst = int(np.argmax(np.where(fr, err / np.maximum(bound, 1e-300), 0.0)))
    report_margin(f"walls with friction {d}D h={h} {which} floor={floor}: node error / (8 u |v|)", float(err[worst]), float(bound[worst]), n=int(fr.sum()))
    assert np.all(err[fr] <= bound[fr]), f"{int((err[fr] > bound[fr]).sum())} frictional nodes over 8 u |v|: worst {err[worst]:.3e} > {bound[worst]:.3e}"
    assert np.array_equal(W.bits(want[~fr]), _u32(vm1[~fr, :d])), "a node outside the frictional faces is not the rule bit for bit"
    assert np.array_equal(_u32(vm1[:, d]), _u32(vm0[:, d]))
    changed = (W.bits(want[fr].astype(np.float32).astype(np.float64)) != _u32(vm0[fr, :d])).any(1)
    assert changed.sum() > 50


# ------------------------------------------------------------------------------------------------ 2. particle by particle
@pytest.mark.parametrize("d,h,which", CASES)
def test_first_substep_particle_by_particle(hip_libs, d, h, which):
    """Fails when k_grid_walls rewrites Dev::nodes alone: the fused G2P stages its velocity tiles from the slabs."""
    sc = _cloud(d, h, which, seed=2)
    ps = sc["particles"]
    walls = _walls(d, which, MIXED[d], friction=0.4, friction_axis=1 if d == 3 else 0)
    _, data = new_data(sc, walls=walls)
    pipeline(d).step(data, 1)
    data.sync()
    cells, vm = data.read_grid()[:2]
    got = data.read_particles()
    inp = T.Inputs.of(ps)
    st, gr, vw, bnd, pt = W.substep(inp, h, T.DT, T.GRAVITY[:d], walls)
    fails = []
    # the node truth itself, with the bound the particle bounds carry
    i = gr.lookup(cells)
    assert (i >= 0).sum() == len(gr.keys)
    hit = i >= 0
    T.check(f"walls {d}D h={h} {which}: walled node velocity", np.linalg.norm(vm[hit, :d].astype(np.float64) - vw[i[hit]], axis=1), bnd[i[hit]], fails)
    T.check_particles(f"walls {d}D h={h} {which} end to end", pt, got, sc["model"], fails)
    iso = T.isolated(inp, st, cells, vm[:, :d], T.DT)
    T.check_particles(f"walls {d}D h={h} {which} isolated G2P", iso, got, sc["model"], fails)
    # the scene does test it: many particles gather wall nodes that 2^D source slabs hold, and the walls change what they get
    m = W.members(gr.cells, walls).any(1)
    touched = m[gr.inv].any(1)
    _, _, pt0 = T.substep(inp, h, T.DT, T.GRAVITY[:d])
    moved = np.linalg.norm(pt.vel - pt0.vel, axis=1) > 10.0 * (pt.b_vel + pt0.b_vel)
    assert touched.sum() > ps.n // 4 and moved.sum() > ps.n // 10, (int(touched.sum()), int(moved.sum()))
    blocks = np.unique(T.assoc_cell(ps.pos, h) // T.bw_of(d), axis=0)
    wall_blocks = np.unique(gr.cells[m] // T.bw_of(d), axis=0)
    have = set(map(tuple, blocks.tolist()))
    full = sum(all(tuple(np.array(b) - np.array(o)) in have for o in np.ndindex(*([2] * d))) for b in map(tuple, wall_blocks.tolist()))
    assert full > 0, "no wall node is gathered from all 2^D source slabs"
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 3. postconditions
@pytest.mark.parametrize("d,h,which", CASES)
def test_postconditions_after_1_2_and_50_substeps(hip_libs, d, h, which):
    sc = _cloud(d, h, which, seed=3, n=4000 if d == 3 else 2000)
    walls = _walls(d, which, MIXED[d], friction=0.25)
    _, data = new_data(sc, walls=walls)
    done = 0
    for upto in (1, 2, 50):
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


@pytest.mark.parametrize("d,h,which", CASES)
def test_a_huge_friction_stops_the_nodes_that_move_into_the_wall(hip_libs, d, h, which):
    sc = _cloud(d, h, which, seed=4, n=4000 if d == 3 else 2000)
    walls = [None] * (2 * d)
    walls[2] = Wall(WALL_SLIP, 1.0e6, PLANES[d, which][1][0])
    walls[3] = Wall(WALL_SEPARATE, 1.0e6, PLANES[d, which][1][1])
    d0, d1 = _twins(sc, walls)
    (c0, vm0), (c1, vm1) = d0.read_grid()[:2], d1.read_grid()[:2]
    assert np.array_equal(c0, c1)
    m = W.members(c0, walls)
    into = (m[:, 2] & (-vm0[:, 1] > 0)) | (m[:, 3] & (vm0[:, 1] > 0))
    assert into.sum() > 50
    assert not vm1[into, :d].any(), f"{int(vm1[into, :d].any(1).sum())} nodes moving into a wall of friction 1e6 keep a velocity"


# ------------------------------------------------------------------------------------------------ 4. containment
@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
@pytest.mark.parametrize("typ", list(TYPES))
def test_a_cloud_thrown_at_every_face_stays_within_a_cell_and_a_half_of_the_planes(hip_libs, d, h, typ):
    """Derived, not measured: a particle with x[k] < (plane - 0.5) h has its whole stencil inside the low face, so its G2P normal
    velocity is >= 0, and the speed cap moves a particle at most h per substep."""
    lo, hi = -3, 13
    sc = scenes.walled_box(d, n=6000 if d == 3 else 2500, lo=lo, hi=hi, wall_type=TYPES[typ], friction=0.2, cell_width=h)
    assert np.abs(sc["particles"].vel).max() > 0.9 * h / sc["params"].dt
    _, data = new_data(sc)
    for _ in range(4):
        pipeline(d).step(data, 50)
        data.sync()
    pos = data.read_positions().astype(np.float64)
    assert np.all(np.isfinite(pos))
    report_margin(f"walled_box {d}D {typ}: furthest beyond a plane (cells)", float(max((lo * h - pos).max(), (pos - hi * h).max()) / h), 1.5 + 1e-3)
    assert pos.min() >= (lo - 1.5) * h - 1e-3 * h and pos.max() <= (hi + 1.5) * h + 1e-3 * h


@pytest.mark.parametrize("d,h", [(2, 0.3), (3, 1.0)])
def test_the_same_cloud_without_walls_leaves_the_box(hip_libs, d, h):
    lo, hi = -3, 13
    sc = scenes.walled_box(d, n=2000, lo=lo, hi=hi, cell_width=h, with_walls=False)
    sc["grid_capacity"] = 32768
    _, data = new_data(sc)
    for _ in range(4):
        pipeline(d).step(data, 10)
        data.sync()
    pos = data.read_positions().astype(np.float64)
    out = ((pos < (lo - 1.5) * h) | (pos > (hi + 1.5) * h)).any(1)
    assert out.mean() > 0.25, f"only {out.mean():.2%} of the cloud left the box: the scene tests nothing"


# ------------------------------------------------------------------------------------------------ 5. same bits
@pytest.mark.parametrize("d,h,which", [(2, 0.3, "B"), (3, 1.0, "A")])
def test_same_bits(hip_libs, monkeypatch, d, h, which):
    sc = _cloud(d, h, which, seed=5, n=4000 if d == 3 else 2000)
    walls = _walls(d, which, MIXED[d], friction=0.3)

    def run(w, remove=False):
        _, data = new_data(sc, walls=w)
        if remove:
            data.set_domain_walls(None)
        pipeline(d).step(data, 20)
        data.sync()
        return data

    a, b = run(walls), run(walls)
    assert _digest(a) == _digest(b)
    ga, gb = a.read_grid()[:2], b.read_grid()[:2]
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(_u32(ga[1]), _u32(gb[1]))
    with debug(monkeypatch, "GU_OWN_LAUNCH"):
        c = run(walls)
    assert _digest(c) == _digest(a), "the walls differ behind the grid update as a launch of its own"
    gc = c.read_grid()[:2]
    assert np.array_equal(ga[0], gc[0]) and np.array_equal(_u32(ga[1]), _u32(gc[1]))
    never, removed = run(None), run(walls, remove=True)
    assert _digest(never) == _digest(removed) != _digest(a)


@pytest.mark.parametrize("d", [2, 3])
def test_getter_and_device_bytes(hip_libs, d):
    sc = _cloud(d, 1.0, "A", n=2000)
    _, data = new_data(sc)
    none = data.domain_walls()
    assert len(none) == 2 * d and all(w.type == WALL_NONE for w in none)
    before = data.stats()["device_bytes"]
    walls = _walls(d, "A", MIXED[d], friction=0.125)
    data.set_domain_walls(walls)
    assert data.domain_walls() == walls
    assert data.stats()["device_bytes"] == before
    pipeline(d).step(data, 2)
    data.sync()
    assert data.stats()["device_bytes"] == before and data.domain_walls() == walls
    part = [walls[0]] + [None] * (2 * d - 1)
    data.set_domain_walls(part)
    assert data.domain_walls()[0] == walls[0] and all(w.type == WALL_NONE for w in data.domain_walls()[1:])
    data.set_domain_walls(None)
    assert all(w == Wall(WALL_NONE, 0.0, 0) for w in data.domain_walls())


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("d", [2, 3])
def test_refusals_change_nothing(hip_libs, d):
    sc = _cloud(d, 1.0, "A", n=2000)
    pipe, data = new_data(sc)
    good = _walls(d, "A", MIXED[d], friction=0.125)
    data.set_domain_walls(good)
    pipe.step(data, 2)
    data.sync()
    digest = _digest(data)
    lib, h = data.lib, data._h

    def arr(f, typ=WALL_SLIP, friction=0.0, plane=0):
        a = (_ffi.Wall * (2 * d))()
        for g, w in enumerate(good):
            a[g].type, a[g].friction, a[g].plane = w.type, w.friction, w.plane
        a[f].type, a[f].friction, a[f].plane = typ, friction, plane
        return a

    lo, hi = good[2].plane, good[3].plane
    bad = [arr(1, typ=4), arr(0, typ=0xffffffff), arr(2, friction=float("nan"), plane=lo), arr(2, friction=float("inf"), plane=lo),
           arr(3, friction=-0.5, plane=hi), arr(2, plane=hi), arr(2, plane=hi + 1), arr(3, plane=lo)]
    invalid, unsupported = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    for a in bad:
        assert lib.wgs_set_domain_walls(h, a) == invalid and lib.wgs_last_error()
        assert data.domain_walls() == good
    assert lib.wgs_get_domain_walls(h, None) == invalid and lib.wgs_set_domain_walls(None, arr(0)) == invalid and lib.wgs_get_domain_walls(None, arr(0)) == invalid
    assert _digest(data) == digest
    # low.plane >= high.plane is refused only where BOTH faces of the axis are set
    one = arr(2, plane=hi + 5)
    one[3].type = WALL_NONE
    assert lib.wgs_set_domain_walls(h, one) == _ffi.WGS_OK
    data.set_domain_walls(good)
    # a lockstep slab: WGS_ERR_UNSUPPORTED, in the words of the other single-domain calls
    shards, _ = lockstep_slabs(pipe, sc, 2)
    for s in shards:
        out = (_ffi.Wall * (2 * d))()
        C.memset(out, 0x5a, C.sizeof(out))
        assert lib.wgs_set_domain_walls(s._h, arr(0)) == unsupported and b"single-domain data only" in lib.wgs_last_error()
        assert lib.wgs_get_domain_walls(s._h, out) == unsupported and bytes(out) == b"\x5a" * C.sizeof(out)
    assert _digest(data) == digest and data.domain_walls() == good


# ------------------------------------------------------------------------------------------------ 7. a tank
@pytest.mark.parametrize("d", [2, 3])
def test_a_tank_of_domain_walls(hip_libs, d):
    """block_in_fluid(walls="grid"): no comparison of values with the collider tank — they are different boundary models."""
    sc = scenes.block_in_fluid(dim=d, walls="grid")
    assert sc["colliders"] == []
    _, data = new_data(sc)
    assert [w.type for w in data.domain_walls()] == [WALL_NONE if w is None else w.type for w in sc["walls"]]
    mass0 = data.diagnostics(_ffi.DIAG_PARTICLES).sums["mass"]
    pipeline(d).step(data, 24)
    data.sync()
    got = data.read_particles()
    for name in ("pos", "vel", "def_grad", "affine"):
        assert np.all(np.isfinite(getattr(got, name))), name
    diag = data.diagnostics(_ffi.DIAG_PARTICLES)
    assert diag.num_nonfinite == 0
    assert np.array_equal(diag.sums["mass"].fixed, mass0.fixed) and diag.sums["mass"].exponent == mass0.exponent
    h = sc["cell_width"]
    for k in ((0,) if d == 2 else (0, 2)):          # the side faces
        lo, hi = sc["walls"][2 * k], sc["walls"][2 * k + 1]
        assert got.pos[:, k].min() >= (lo.plane - 1.5) * h - 1e-3 * h and got.pos[:, k].max() <= (hi.plane + 1.5) * h + 1e-3 * h
    assert got.pos[:, 1].min() >= (sc["walls"][2].plane - 1.5) * h - 1e-3 * h
    fields = data.particle_fields()
    assert fields.stress.shape == (got.n, d, d) and np.all(np.isfinite(fields.stress)) and np.all(np.isfinite(fields.volume_ratio))
