"""-m gpu: what P2G, G2P and the particle update do with the collider distance fields (the CPIC transfer), checked node by node
and particle by particle against the fp64 truth of tests/cpic_truth.py (its bounds are validated on the CPU by
tests/test_cpic_truth.py). gpu_common.checked_cpic_substep runs one substep and checks the distance fields
(tests/cdf_truth.py) and then, from the kernel's own decisions, every node's mass and velocity and every particle's x, v, F
and C' twice: from the kernel's own grid and end to end.

Scenes: tests/cpic_truth.py's (moving colliders with the centre of mass off the translation, uploaded previous affinity
words, near-tangential relative velocities, a thin plate, 16 collider slots), each launch shape of the CPIC passes, a
steady-state substep of a stirred bed on a floor with a ball driven into it, colliders at rest (the one-way P2G: every other
scene has a collider with a velocity, which makes the library launch the two-way instantiation), a dynamic cuboid, and two
lockstep slabs of the bed whose cut runs through the contact layer (the arrivals' kernel).

The case is in the test id, not in the check names: tools/summarize_margins.py then gives the worst record per check."""
import contextlib
import dataclasses

import numpy as np
import pytest

import cdf_truth as CT
import cpic_truth as CP
import transfer_truth as T
from gpu_common import _bed_scene, checked_cpic_substep, export_state_and_cdf
from helpers import debug, new_data, pipeline, report_margin
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider, SimulationParams

pytestmark = pytest.mark.gpu

CASES = [(name, d, h) for name in CP.SCENES for d in (2, 3) for h in CP.HS]
SHAPES = ("P2G_TWO_LAUNCHES", "G2P_TWO_LAUNCHES", "NO_PCDF_WAVES", "G2P_TWO_PASSES", "NO_DIRECT_RUNS")


def _scene(name, d, h, **kw):
    sc = CP.SCENES[name](d, h, **kw)
    sc["colliders"] = sc["colliders"][:16]           # (sixteen: the library refuses a 17th collider, tests/test_gpu_cdf.py)
    return sc


def _report_reach(tag, res):
    r = CP.reach(res)
    report_margin(f"{tag}: incompatible (particle, node) pairs", r["incompatible_pairs"], 0)
    report_margin(f"{tag}: penetrating particles", r["penetrating"], 0, deeper_than_the_clamp=r["deeper_than_clamp"])
    return r


@pytest.mark.parametrize("name,d,h", CASES)
def test_one_substep_node_by_node_and_particle_by_particle(hip_libs, name, d, h):
    i = CASES.index((name, d, h))
    sc = _scene(name, d, h, model=i % 2, uniform=i % 2 == 1)          # (the two layouts alternate)
    data = new_data(sc)[1]
    fails = []
    tag = "cpic one substep"
    res = checked_cpic_substep(tag, sc, data, fails, first=True).end_to_end
    r = _report_reach(tag, res)
    assert not fails, "\n".join(fails)
    assert r["incompatible_pairs"] >= 1000 and r["penetrating"] >= 30, r
    if name == "sixteen":
        assert r["closest_ids"] == list(range(16)), r


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("switch", SHAPES)
def test_each_launch_shape_of_the_cpic_passes(hip_libs, monkeypatch, switch, d):
    """the two P2G bodies and the two G2P bodies as two launches each, the particle cdf inside the CPIC workgroups, two chunks
    per wave of the fused G2P, P2G through the permutation; the bit-identity tests tie the remaining shapes to these"""
    h = 0.5
    sc = _scene("two_equal", d, h)
    with debug(monkeypatch, switch):
        data = new_data(sc)[1]
    fails = []
    tag = "cpic launch shape"
    res = checked_cpic_substep(tag, sc, data, fails, first=True).end_to_end
    r = _report_reach(tag, res)
    assert not fails, "\n".join(fails)
    assert r["incompatible_pairs"] >= 1000 and r["only_incompatible_nodes"] >= 1, r


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("switch", [None, "P2G_TWO_LAUNCHES", "NO_DIRECT_RUNS"])
@pytest.mark.parametrize("name,h", [("two_equal", 0.5), ("cuboid", 0.2)])
def test_colliders_at_rest_take_the_one_way_p2g(hip_libs, monkeypatch, name, h, switch, d):
    """No collider has a velocity or a mass, so the library launches the one-way instantiations of the CPIC P2G (a body of
    its own in the compiled code), as one launch with the plain P2G and as a launch of its own. The uploaded previous words
    still give incompatible pairs and penetration; the ghost velocities are project(v_p, n)."""
    sc = _scene(name, d, h, fixed=True)
    assert not any(np.any(c.linvel) or np.any(c.angvel) or np.any(c.inv_mass) for c in sc["colliders"])
    with debug(monkeypatch, switch) if switch else contextlib.nullcontext():
        data = new_data(sc)[1]
    fails = []
    tag = "cpic colliders at rest"
    ck = checked_cpic_substep(tag, sc, data, fails, first=True)
    r = _report_reach(tag, ck.end_to_end)
    assert not fails, "\n".join(fails)
    assert r["incompatible_pairs"] >= 1000 and r["penetrating"] >= 30 and min(r["stick"], r["slide"], r["away"]) >= 10, r
    after = data.read_body_poses()
    assert all(not p["linvel"].any() and not p["angvel"].any() for p in after)


def _drive(sc, data, d, h):
    """the host pushes the ball 0.3 h further into the bed (beyond the 0.09 h its own velocity moves it per substep: a body
    in contact is limited to 0.1 h): the particles at its surface keep their sign, and find themselves on the other side"""
    floor, ball = sc["colliders"]
    tr = np.asarray(data.read_body_poses()[1]["translation"], np.float64)
    tr[1] -= 0.3 * h
    data.set_colliders([floor, dataclasses.replace(ball, translation=tuple(float(v) for v in CT.f32(tr)))])


@pytest.mark.parametrize("d", [2, 3])
def test_steady_state_substep(hip_libs, d):
    """8 substeps, then five before each of which the host pushes the ball, then one without a push; the last two are checked,
    each from the state read back. A push goes through set_colliders, which makes every kept node cdf and block class stale:
    the 13th substep is steady on the particles' side only (clean and dirty blocks, k_regroup's arrivals, the binning inside
    the fused G2P), the 14th on the cdf side too (node cdfs kept where the ball's own motion leaves them valid). In both the
    particles penetrate by the sign they earned themselves: no previous affinity word was uploaded."""
    h = 0.2 if d == 2 else 0.25
    sc = _bed_scene(d, h)
    data = new_data(sc)[1]
    pipeline(d).step(data, 8)
    for _ in range(4):
        data.sync()
        _drive(sc, data, d, h)
        pipeline(d).step(data, 1)
    data.sync()
    _drive(sc, data, d, h)
    fails = []
    for tag in ("cpic steady state, the ball just pushed", "cpic steady state"):
        s0 = data.stats()
        ck = checked_cpic_substep(tag, sc, data, fails, first=False)
        s1 = data.stats()
        r = _report_reach(tag, ck.end_to_end)
        report_margin(f"{tag}: cell changers in the checked substep", s1["cell_changers"] - s0["cell_changers"], 0)
        report_margin(f"{tag}: near-collider blocks", s1["num_near_collider_blocks"], 0)
        assert s1["table_rebuilds"] == s0["table_rebuilds"], "the checked substep rebuilt the table: not a steady-state substep"
        assert s1["cell_changers"] > s0["cell_changers"], "no particle changed cell in the checked substep"
        assert s1["num_near_collider_blocks"] > 0
        assert r["penetrating"] >= 10 and r["deeper_than_clamp"] >= 5 and r["incompatible_pairs"] >= 100, r
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d", [2, 3])
def test_dynamic_body(hip_libs, d):
    """A cuboid of finite mass among the particles. Its P2G is the two-way instantiation every scene with a moving collider
    runs (the kinematic ones too); what sets this case apart is that the impulses the incompatible pairs leave move the body:
    its angular velocity, which nothing else changes, differs after the substep. Grid and particles are checked against the
    velocities the body had before it; what the body receives and how it integrates is checked by tests/test_gpu_bodies.py
    (gpu_common.checked_body_substep, against tests/body_truth.py)."""
    h = 0.2
    sc = _scene("cuboid", d, h)
    sc["colliders"] = [dataclasses.replace(c.with_density(50.0, d), linvel=c.linvel, angvel=c.angvel) for c in sc["colliders"]]
    data = new_data(sc)[1]
    fails = []
    tag = "cpic dynamic body"
    before = data.read_body_poses()
    res = checked_cpic_substep(tag, sc, data, fails, first=True).end_to_end
    r = _report_reach(tag, res)
    assert not fails, "\n".join(fails)
    assert r["incompatible_pairs"] >= 1000 and r["penetrating"] >= 30, r
    assert np.abs(res.grid.dimp).max() > 0.0
    assert not np.array_equal(data.read_body_poses()[0]["angvel"], before[0]["angvel"]), "the body took no impulse"


@pytest.mark.parametrize("d", [2, 3])
def test_lockstep_slabs_particle_by_particle(hip_libs, d):
    """A denser bed of the steady-state test drifting along x at 0.5 h per substep, as two lockstep slabs: the cut under the
    ball and through the contact layer of the floor. Every particle of substeps 9 to 13 (the ball pushed by the host before
    each) end to end against the truth of the whole domain (its nodes' affinities and closest ids from
    cdf_truth.NodeField; particles that touch an undecided node are left out, under PART_CAP); the arrivals (particles a rank
    holds outside its core range: the arrivals' kernel transfers them) on their own."""
    from wgsparkl_amd.sharded import associated_block_x, native_lockstep
    h = 0.2 if d == 2 else 0.25
    sc = _bed_scene(d, h, n=12000 if d == 2 else 6000, drift=0.5)
    ps = sc["particles"]
    pipe = pipeline(d)
    shards, part = lockstep_slabs(pipe, sc, 2)
    lo_hi = np.array([part.block_range(r) for r in range(2)])

    def run(k):
        native_lockstep(pipe, shards, k)
        for s in shards:
            s.sync()

    run(8)
    pre, holder = export_state_and_cdf(shards, ps.n, d)[:2]
    fails = []
    n_arr = n_contact = n_out = n_reach = n_pen = near = 0
    for step in range(8, 13):
        for s in shards:
            _drive(sc, s, d, h)
        poses = shards[0].read_body_poses()
        run(1)
        post, held, aff, dist, normal = export_state_and_cdf(shards, ps.n, d)
        inp = T.Inputs(pre["pos"], pre["vel"], pre["affine"], pre["def_grad"], pre["mass"], ps.init_volume, ps.lambda_, ps.mu)
        nf = CT.NodeField(CT.colliders_of(sc["colliders"], d, poses), d, h, CT.active_cells(inp.pos32, h, d))
        f = CP.Fields(aff, normal.astype(np.float64), dist.astype(np.float64), nf.cells, nf.aff, nf.closest)
        res = CP.substep(inp, h, T.DT, T.GRAVITY[:d], f, CP.Motion.of(sc["colliders"], d, poses), extra_levels=8.0)
        und = nf.undecided | nf.und_dist
        touches = und[np.searchsorted(nf.keys, T.node_key(res.st.node.reshape(-1, d)))].reshape(ps.n, -1).any(1)
        reaches = (aff != 0) | (~res.compat).any(1)
        bx = associated_block_x(inp.pos32, h, d)
        arrival = (bx < lo_hi[holder, 0]) | (bx >= lo_hi[holder, 1])
        contact_arrival = arrival & (~res.compat).any(1) & ~touches
        tag = "cpic slabs"
        near += CP.check_result(f"{tag} all", res, None, None, post, sc["model"], fails, extra_levels=8.0, sel=~touches)[2]
        CP.check_result(f"{tag} arrivals", res, None, None, post, sc["model"], fails, extra_levels=8.0, sel=arrival & ~touches)
        CP.check_result(f"{tag} arrivals incompatible with some node", res, None, None, post, sc["model"], fails, extra_levels=8.0, sel=contact_arrival)
        n_arr += int(arrival.sum())
        n_contact += int(contact_arrival.sum())
        n_out += int((touches & reaches).sum())
        n_reach += int(reaches.sum())
        n_pen += int((res.contact.pen & ~touches).sum())
        pre, holder = post, held
    for s in shards:
        s.close()
    report_margin(f"{tag}: particles left out (they touch an undecided node), of those that reach a collider", n_out / max(n_reach, 1), CT.PART_CAP, count=n_out)
    report_margin(f"{tag}: arrivals in the checked substeps", n_arr, 0, incompatible_with_some_node=n_contact, penetrating=n_pen)
    CP.assert_near(tag, 0, 0, near, 5 * ps.n)
    assert not fails, "\n".join(fails)
    assert n_out <= CT.PART_CAP * n_reach, (n_out, n_reach)
    assert n_contact >= 10 and n_pen >= 10, (n_arr, n_contact, n_pen)
