"""CPU: the fp64 truth of what the rigid bodies receive and how they integrate (tests/body_truth.py) and its bounds are right.

- the C oracle run pass by pass with its bodies (body_truth.oracle_substep): the fp32 oracle's accumulators lie in the truth's
  integer interval and its bodies within the truth's bounds; the fp64 oracle within the same bounds at u = 2^-53 (the fixed-point
  conversions are fp32 in both: their terms stay multiples of 2^-24);
- the scenes reach what their bodies are named after (body_truth.ROLES) and stay in the int32 range;
- each of thirteen wrong rules, a named variant of the truth, rejects the fp32 oracle's output on some scene;
- `cuboid` at h = 2.0 leaves the int32 range: the oracle's accumulators are those of the truth's saturate-then-wrap arithmetic;
- sixteen free bodies integrate within the bounds over 1 and 50 substeps.

Sensitivity (body_truth.sensitivity: the share of a body's contributing nodes that a velocity check would see one by one) is
asserted >= 0.9 on every axis for every body below the caps, in every case. That is a condition on the inputs which cpic_truth's
five scenes cannot meet with any mass (their bodies collect 30 to 300 node totals spanning five orders of magnitude under
near-equal node bounds, and only the sum is observable), so here their dynamic bodies are light enough to end on a cap and the
bodies below the caps are those of the `lone` scenes: one particle against a ball, a rotated cuboid of unequal inertia, a
body with a locked axis, in both dimensions, and `quantum` in 2D."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

import body_truth as BT
import cdf_truth as CT
import cpic_truth as CP
import transfer_truth as T

CASES = BT.CASES


class Run(NamedTuple):
    sc: dict
    ob: BT.OracleBodies
    inp: T.Inputs
    motion: CP.Motion
    res: CP.Result
    props: BT.Props


def _truth(sc, ob, u):
    d, h = sc["particles"].dim, sc["cell_width"]
    inp = T.Inputs.of(sc["particles"])
    mo = CP.Motion.of(sc["colliders"], d, ob.before)
    res = CP.substep(inp, h, T.DT, sc["params"].gravity, ob.run.fields, mo, u=u)
    return Run(sc, ob, inp, mo, res, BT.Props(sc["colliders"], d))


@functools.lru_cache(maxsize=None)
def _run(name, d, h):
    i = CASES.index((name, d, h))
    sc = BT.BUILD[name](d, h, model=i % 2, uniform=i % 2 == 1)       # (as tests/test_gpu_bodies.py builds them: the two layouts alternate)
    return _truth(sc, BT.oracle_substep(sc, np.float32), T.U32)


def _check(tag, r: Run, fails, u=T.U32, variant=()):
    sc = r.sc
    imp = BT.impulses(r.res, r.inp, r.motion, u, variant)
    BT.check_accumulators(tag, imp, r.ob.acc[:r.props.n], fails)
    ck = BT.check_bodies(tag, imp, r.props, r.ob.before, r.ob.after, sc["cell_width"], T.DT, sc["params"].gravity, fails, u=u, variant=variant)
    return imp, ck


@pytest.mark.parametrize("name,d,h", CASES)
def test_the_oracles_fit_the_bounds_and_the_scene_reaches_its_roles(oracle_libs, name, d, h):
    r = _run(name, d, h)
    tag = f"bodies {name} {d}D h={h}"
    fails = []
    r64 = _truth(r.sc, BT.oracle_substep(r.sc, np.float64), T.U64)
    imp64, _ = _check(f"{tag} fp64 oracle", r64, fails, u=T.U64)
    assert not fails, "\n".join(fails)
    imp, ck = _check(f"{tag} fp32 oracle", r, fails)
    assert not fails, "\n".join(fails)
    assert imp.in_range and imp64.in_range, tag
    assert ck.near == 0, (tag, "a body of the CPU scenes is near a cap")
    below = BT.reached(tag, r.sc, imp, ck, r.ob.before, r.ob.after)
    # every body below the caps that can take an impulse, whatever its role: each of its nodes is visible in a velocity
    assert set(below) <= set(BT.assert_sensitive(tag, ck))
    assert below or not name.startswith("lone")
    if name == "sixteen":
        assert sorted(set(imp.body[np.abs(imp.tot).sum(1) > 0].tolist())) == list(range(16)), "not every one of the 16 bodies receives an impulse"


def test_the_scene_set_provides_every_kind_of_body(oracle_libs):
    roles = {role for name in BT.BUILD for role in BT.ROLES[name]}
    assert {"below", "linear_cap", "angular_cap", "fast_touched", "fast_untouched", "locked_y", "kinematic", "light"} <= roles
    # a rotated 3D cuboid whose world and local inverse inertia differ, the centre of mass off the translation
    r = _run("lone_cuboid", 3, 0.2)
    body = BT.integrate(BT.State.of(r.ob.before[0]), r.props.inv_mass[0], r.props.inv_inertia[0], np.zeros(6), np.zeros(6), 0.2, T.DT, T.GRAVITY)
    assert np.abs(body.inertia_world - r.props.inv_inertia[0]).max() > 0.1 * np.abs(r.props.inv_inertia[0]).max()
    assert np.linalg.norm(r.ob.before[0]["com"] - r.ob.before[0]["translation"]) > 0.5 * 0.2


SEARCH = sorted(CASES, key=lambda c: (c[0] != "quantum", c[1], c[2]))


@pytest.mark.parametrize("variant", BT.VARIANTS)
def test_a_wrong_rule_rejects_the_fp32_oracle(oracle_libs, variant):
    """the truth restated with the wrong rule no longer holds the fp32 oracle's accumulators or bodies, in some scene"""
    for name, d, h in SEARCH:
        fails = []
        _check(f"{variant} {name} {d}D h={h}", _run(name, d, h), fails, variant=(variant,))
        if fails:
            return
    pytest.fail(f"{variant}: the fp32 oracle fits the wrong rule's bounds in every scene")


@pytest.mark.parametrize("d", [2, 3])
def test_out_of_range_saturates_and_wraps_like_the_oracle(oracle_libs, d):
    """cuboid at h = 2.0 with the mass of density 50: node totals beyond 2^31 units saturate, the sums wrap modulo 2^32"""
    sc = BT.out_of_range(d)
    r = _truth(sc, BT.oracle_substep(sc, np.float32), T.U32)
    imp = BT.impulses(r.res, r.inp, r.motion)
    assert not imp.in_range
    assert (np.abs(imp.lo) >= (1 << 31)).any() or imp.saturating.any(), "neither a wrap nor a saturation"
    # (the interval covers less than an eighth of the ring on every axis: an accumulator computed otherwise lands in it by chance at most that often)
    assert ((imp.hi - imp.lo) < (1 << 29)).all(), "an interval too wide to say anything modulo 2^32"
    fails = []
    BT.check_accumulators(f"bodies out of range {d}D", imp, r.ob.acc[:1], fails)
    BT.check_bodies(f"bodies out of range {d}D", imp, r.props, r.ob.before, r.ob.after, 2.0, T.DT, sc["params"].gravity, fails)
    assert not fails, "\n".join(fails)
    BT.report_margin(f"bodies out of range {d}D: saturating node totals", int(imp.saturating.sum()), 0, largest_sum=float(np.abs(imp.lo).max()))


@pytest.mark.parametrize("count", [1, 50])
@pytest.mark.parametrize("d", [2, 3])
def test_free_bodies_integrate_within_bounds(oracle_libs, d, count):
    """no impulse, no cap: velocities, poses and centres of mass of sixteen free bodies after `count` substeps against the
    integration truth iterated in fp64, the bound `count` times that of the last substep"""
    sc = BT.free_bodies(d)
    from helpers import oracle
    ps = sc["particles"]
    st = oracle(d, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    st.update_world_mass_properties()
    before = st.collider_states()
    st.step(count)
    st.update_world_mass_properties()
    fails = []
    after = st.collider_states()
    BT.check_free(f"free bodies {d}D x{count} fp32 oracle", sc, before, after, count, fails)
    assert not fails, "\n".join(fails)
    # the fixed rotated collider keeps its pose bit for bit (the oracle has no shortcut for a body at rest: this rotation is one its
    # renormalisation returns unchanged; the kernels guarantee it for every rotation, tests/test_gpu_bodies.py)
    k = sc["fixed"]
    assert all(np.array_equal(after[k][q], before[k][q]) for q in before[k]), "the fixed collider moved"
