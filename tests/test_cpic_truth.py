"""CPU: the fp64 truth of the CPIC transfer (tests/cpic_truth.py) and its bounds are right.

- fed the C fp64 oracle's own cdf fields (the oracle run pass by pass), the truth agrees with that oracle's grid and
  particles per element at u = 2^-53;
- fed the C fp32 oracle's own cdf fields, the C fp32 oracle lands inside every bound: the grid, the particles end to end, the
  particles from its own grid; the share of particles near the speed cap or a threshold of sd stays below NEAR_MAX;
- the scenes reach what they are built for (incompatible pairs, several affinity bits, nodes reached by incompatible pairs
  only, penetration on both sides of -0.3 h, every branch of project_velocity, all 16 collider slots);
- each of thirteen wrong rules, a named variant of the truth, moves the fp32 oracle's output outside a bound: in some case
  at least 10 elements of one check (nodes, or particles in one of x, v, F, C') exceed their bound more than tenfold."""
import functools

import numpy as np
import pytest

import cpic_truth as CP
import transfer_truth as T

CASES = [(name, d, h) for name in CP.SCENES for d in (2, 3) for h in CP.HS]
# the cases a variant is looked for in, the small ones first
SEARCH = sorted(CASES, key=lambda c: (c[1], c[0] not in ("two_equal", "sixteen"), c[2] != 0.5))


def _model(d, h):
    return (d + int(h * 10)) % 2                      # both models over the cases


@functools.lru_cache(maxsize=None)
def _run(name, d, h, fixed=False):
    model = _model(d, h)
    sc = CP.SCENES[name](d, h, model=model, fixed=fixed)
    inp = T.Inputs.of(sc["particles"])
    mo = CP.Motion.of(sc["colliders"], d)
    o32 = CP.oracle_substep(sc, np.float32)
    res = CP.substep(inp, h, T.DT, sc["params"].gravity, o32.fields, mo)
    return sc, inp, mo, o32, res, model


@pytest.mark.parametrize("name,d,h", CASES)
def test_truth_matches_the_fp64_oracle_and_the_fp32_oracle_fits_the_bounds(oracle_libs, name, d, h):
    sc, inp, mo, o32, res, model = _run(name, d, h)
    g = sc["params"].gravity
    tag = f"cpic {name} {d}D h={h}"
    fails = []
    o64 = CP.oracle_substep(sc, np.float64)
    r64 = CP.substep(inp, h, T.DT, g, o64.fields, mo, u=T.U64)
    CP.check_result(f"{tag} fp64 oracle", r64, o64.cells, o64.vm, o64.arr, model, fails, u=T.U64)
    assert not fails, "\n".join(fails)
    near_n, nn, near_p = CP.check_result(f"{tag} fp32 oracle end to end", res, o32.cells, o32.vm, o32.arr, model, fails)
    iso = CP.substep(inp, h, T.DT, g, o32.fields, mo, own_grid=(o32.cells, o32.vm[:, :d]))
    CP.check_result(f"{tag} fp32 oracle isolated G2P", iso, None, None, o32.arr, model, fails)
    # the velocity bound term by term: which particles pay which constants (rigid_vel itself, C_BODY alone, is checked above)
    pt, ghost, pen = res.particles, (~res.compat).any(1), res.contact.pen
    err = np.linalg.norm(np.asarray(o32.arr["vel"], np.float64) - pt.vel, axis=1)
    T.check("cpic fp32 oracle: v, compatible nodes only, not penetrating (C_G2P, the node bounds)", err, pt.b_vel, fails, ~ghost & ~pen & ~res.contact.near_pen)
    T.check("cpic fp32 oracle: v, some ghost velocity, not penetrating (+ C_BODY, C_PROJ, L once)", err, pt.b_vel, fails, ghost & ~pen & ~res.contact.near_pen)
    T.check("cpic fp32 oracle: v, penetrating (+ rigid_vel, C_PROJ, L again, C_PEN)", err, pt.b_vel, fails, pen & ~res.contact.near_pen)
    assert not fails, "\n".join(fails)
    CP.assert_near(tag, near_n, nn, near_p, inp.n)


@pytest.mark.parametrize("d", [2, 3])
def test_fixed_colliders_fit_as_well(oracle_libs, d):
    """the scenes with every collider at rest (what runs the one-way P2G of the library): ghost velocities are project(v_p, n)"""
    name, h = "two_equal", 0.5
    sc, inp, mo, o32, res, model = _run(name, d, h, fixed=True)
    assert not mo.linvel.any() and not mo.angvel.any()
    fails = []
    tag = f"cpic fixed {name} {d}D h={h}"
    near_n, nn, near_p = CP.check_result(f"{tag} fp32 oracle end to end", res, o32.cells, o32.vm, o32.arr, model, fails)
    iso = CP.substep(inp, h, T.DT, sc["params"].gravity, o32.fields, mo, own_grid=(o32.cells, o32.vm[:, :d]))
    CP.check_result(f"{tag} fp32 oracle isolated G2P", iso, None, None, o32.arr, model, fails)
    assert not fails, "\n".join(fails)
    CP.assert_near(tag, near_n, nn, near_p, inp.n)
    r = CP.reach(res)
    assert r["incompatible_pairs"] >= 1000 and r["only_incompatible_nodes"] >= 1 and r["penetrating"] >= 30, r
    assert min(r["away"], r["stick"], r["slide"]) >= 10, r


@pytest.mark.parametrize("name,d,h", CASES)
def test_the_scenes_reach_what_they_are_built_for(oracle_libs, name, d, h):
    sc, inp, mo, o32, res, _ = _run(name, d, h)
    r = CP.reach(res)
    assert r["incompatible_pairs"] >= 1000 and r["particles_with_incompatible"] >= 300, r
    if name in ("two_equal", "ball", "sixteen"):
        assert r["multi_affinity"] >= 400, r
    if name in ("two_equal", "sixteen") and (d == 2 or h == 0.5):
        assert r["only_incompatible_nodes"] >= 1, r
    # (sixteen's balls are smaller than a cell: few particles lie deep by their stored sign)
    deep, shallow = (30, 3) if name == "sixteen" else (90, 20)
    assert r["deeper_than_clamp"] >= deep and r["penetrating"] - r["deeper_than_clamp"] >= shallow, r
    assert min(r["away"], r["stick"], r["slide"]) >= 10, r
    if name == "sixteen":
        assert len(sc["colliders"]) == 17 and r["closest_ids"] == list(range(16)), r
    # moving colliders as a body in contact is capped: every component non-zero, the centre of mass off the translation
    lim = 0.1 * h / T.DT
    assert np.all(mo.linvel != 0) and np.all(mo.angvel != 0) and np.all(mo.com != mo.trans)
    assert np.all(np.linalg.norm(mo.linvel, axis=1) <= lim) and np.all(np.linalg.norm(mo.angvel, axis=1) <= 1.0)
    # the near-tangential subset: relative velocity with a normal part below 1/20 of the tangential part, on both sides of h / dt
    f = o32.fields
    rel = inp.v - res.contact.rigid_vel
    nv = np.einsum("nk,nk->n", rel, f.pnormal)
    tl = np.linalg.norm(rel - f.pnormal * nv[:, None], axis=1)
    tang = (f.paff != 0) & (nv < 0) & (np.abs(nv) < tl / 20.0)
    fast = 0 if name in CP.SPEED else 5
    assert tang.sum() >= 30 and (tang & (tl > h / T.DT)).sum() >= fast and (tang & (tl < h / T.DT)).sum() >= 5, int(tang.sum())


def _moved(o32, res, bad, model, d):
    """the fp32 oracle's output moved by (variant - truth)"""
    gr, pt = res.grid, res.particles
    vm = o32.vm.copy()
    i = gr.lookup(o32.cells)
    ok = i >= 0
    vm[ok, :d] += (bad.grid.vel - gr.vel)[i[ok]]
    vm[ok, d] += (bad.grid.mass - gr.mass)[i[ok]]
    got = dict(o32.arr)
    F = o32.arr["def_grad"]
    for k, delta in (("pos", bad.particles.x - pt.x), ("vel", bad.particles.vel - pt.vel), ("def_grad", T.unmat(bad.particles.F - pt.F)),
                     ("affine", T.unmat(bad.particles.affine(model, F)[0] - pt.affine(model, F)[0]))):
        got[k] = np.asarray(o32.arr[k], np.float64) + delta
    return vm, got


@pytest.mark.parametrize("variant", CP.VARIANTS)
def test_a_wrong_rule_breaks_the_bounds(oracle_libs, variant):
    best = (0, None)
    for name, d, h in SEARCH:
        sc, inp, mo, o32, res, model = _run(name, d, h)
        bad = CP.substep(inp, h, T.DT, sc["params"].gravity, o32.fields, mo, variant=(variant,))
        vm, got = _moved(o32, res, bad, model, d)
        ex = CP.excess(res, o32.cells, vm, got, model)
        over = {k: int((v > 10.0).sum()) for k, v in ex.items()}     # (per check: x and v of one particle are not two elements)
        if max(over.values()) > best[0]:
            best = (max(over.values()), (name, d, h, over))
        if best[0] >= 10:
            break
    assert best[0] >= 10, f"{variant}: at most {best[0]} elements of one check exceed their bound tenfold ({best[1]})"
