"""CPU: the fp64 transfer truth of tests/transfer_truth.py and its bounds are right.

- the truth agrees per element with the C fp64 oracle (the same bounds at u = 2^-53: a few 1e-15 of the stated scales);
- the C fp32 oracle, an honest fp32 implementation with another summation order, lands inside every bound (grid, particles
  end to end, particles from its own grid through the isolated G2P truth): the bounds are not too tight;
- single-element perturbations of the fp32 oracle's output land outside them: the bounds are not vacuous."""
import numpy as np
import pytest

import transfer_truth as T
from helpers import grid_of, run_oracle

CASES = [(name, d, h) for name in T.SCENES for d in (2, 3) for h in (0.2, 0.3, 0.5, 2.0)]


def _run(name, d, h, model=0):
    sc = T.SCENES[name](d, h, model=model)
    inp = T.Inputs.of(sc["particles"])
    return sc, inp, run_oracle(sc, 1, np.float32), run_oracle(sc, 1, np.float64)


def _grid(st):
    cells, mv = grid_of(st)[:2]
    return cells, mv


@pytest.mark.parametrize("name,d,h", CASES)
def test_truth_matches_the_fp64_oracle_and_the_fp32_oracle_fits_the_bounds(oracle_libs, name, d, h):
    model = (d + int(h * 10)) % 2                      # both models over the cases
    sc, inp, st32, st64 = _run(name, d, h, model)
    g = sc["params"].gravity
    # fp64: the truth against the C fp64 oracle, node by node and particle by particle
    fails = []
    _, gr64, pt64 = T.substep(inp, h, T.DT, g, u=T.U64)
    T.check_grid(f"{name} {d}D h={h} fp64 oracle", gr64, *_grid(st64), fails, u=T.U64)
    T.check_particles(f"{name} {d}D h={h} fp64 oracle", pt64, st64.arr, model, fails)
    assert not fails, "\n".join(fails)
    # fp32: the C fp32 oracle inside every bound
    st, gr, pt = T.substep(inp, h, T.DT, g)
    cells, mv = _grid(st32)
    T.check_grid(f"{name} {d}D h={h} fp32 oracle", gr, cells, mv, fails)
    T.check_particles(f"{name} {d}D h={h} fp32 oracle end to end", pt, st32.arr, model, fails)
    iso = T.isolated(inp, st, cells, mv[:, :d], T.DT)
    T.check_particles(f"{name} {d}D h={h} fp32 oracle isolated G2P", iso, st32.arr, model, fails)
    assert not fails, "\n".join(fails)


def test_the_scenes_reach_the_edges_they_are_named_for():
    # ties at power-of-two h are exact: weights of exactly 0 (nodes of zero truth mass inside active blocks)
    inp = T.Inputs.of(T.ties(3, 0.5)["particles"])
    st = T.Stencil(inp, 0.5)
    assert (st.w == 0.0).any()
    # h = 0.2: positions where round(x / h) and round(x * (1 / h)) differ in fp32
    assert T.division_rule_differs(T.ties(3, 0.2)["particles"].pos, 0.2).sum() >= 10
    assert T.division_rule_differs(T.ties(2, 0.2)["particles"].pos, 0.2).sum() >= 10
    # coordinates: both signs, and blocks two inside the packed key range
    for d, lo, hi in ((3, (-1021, -509, -1021), (1022, 510, 1022)), (2, (-32765, -32765), (32766, 32766))):
        pos = T.coordinates(d, 1.0)["particles"].pos
        blk = T.assoc_cell(pos, 1.0) // T.bw_of(d)
        assert np.array_equal(blk.min(0), lo) and np.array_equal(blk.max(0), hi)
        assert ((pos < 0).any(0) & (pos > 0).any(0)).all()
    # clamps: node velocities on both sides of h / dt
    sc = T.clamps(3, 0.5)
    _, gr, pt = T.substep(T.Inputs.of(sc["particles"]), 0.5, T.DT, T.GRAVITY)
    a = np.abs(gr.vel_u[gr.mass > 0])
    assert (a > gr.lim).any() and ((a < gr.lim) & (a > 0.5 * gr.lim)).any()
    assert (np.linalg.norm(pt.vel_g, axis=1) > pt.lim).any() and (np.linalg.norm(pt.vel_g, axis=1) < pt.lim).any()
    # source patterns: 15 / 255 islands, every subset of the 2^d sources
    for d, n in ((2, 15), (3, 255)):
        pos = T.source_patterns(d, 1.0)["particles"].pos
        assert len(pos) >= n


def _fails_grid(gr, cells, mv):
    f = []
    T.check_grid("perturbed", gr, cells, mv, f)
    return f


@pytest.mark.parametrize("d", [2, 3])
def test_perturbations_of_the_fp32_oracle_break_the_bounds(oracle_libs, d):
    h = 0.5
    sc, inp, st32, _ = _run("source_patterns", d, h)
    g = sc["params"].gravity
    st, gr, pt = T.substep(inp, h, T.DT, g)
    cells, mv = _grid(st32)
    assert not _fails_grid(gr, cells, mv)
    row = {k: i for i, k in enumerate(T.node_key(cells))}
    # a node with a few contributors; its largest contribution
    node = int(np.argmax(np.where(gr.count >= 2, gr.mass, 0.0)))
    p, s = np.argwhere(gr.inv == node)[np.argmax(st.w[gr.inv == node] * inp.m[np.nonzero(gr.inv == node)[0]])]
    wm = st.w[p, s] * inp.m[p]
    r = row[int(gr.keys[node])]

    def node_with(mass, mom_delta):
        out = mv.copy()
        m32 = mv[r, d]
        mom = mv[r, :d] * m32 - m32 * np.asarray(g[:d]) * T.DT + mom_delta
        out[r, d] = mass
        out[r, :d] = np.clip((mom + mass * np.asarray(g[:d]) * T.DT) / mass, -gr.lim, gr.lim)
        return out

    contrib = (inp.C[p] @ st.dpt[p, s] + inp.m[p] * inp.v[p]) * st.w[p, s]
    # one particle dropped from one node
    assert _fails_grid(gr, cells, node_with(mv[r, d] - wm, -contrib))
    # one weight scaled by (1 + 1e-4)
    assert _fails_grid(gr, cells, node_with(mv[r, d] + 1e-4 * wm, 1e-4 * contrib))
    # 4 in place of 4 / h^2 (h = 0.5): C' of the particles
    bad = T.Particles(inp, st, gr.vel[gr.inv], T.DT, variant=("invd_4",))
    got = dict(st32.arr)
    got["affine"] = (st32.arr["affine"] + T.unmat(bad.affine(0, st32.arr["def_grad"])[0] - pt.affine(0, st32.arr["def_grad"])[0])).astype(np.float32)
    f = []
    T.check_particles("perturbed", pt, got, 0, f)
    assert f and all("C'" in x for x in f)
    # g[1] on every axis
    bad = T.Grid(inp, st, T.DT, g, variant=("gravity_g1_on_every_axis",))
    assert _fails_grid(gr, cells, _moved(mv, gr, bad, cells, d))


@pytest.mark.parametrize("d", [2, 3])
def test_a_clamp_of_one_over_dt_breaks_the_bounds(oracle_libs, d):
    h = 0.5
    sc, inp, st32, _ = _run("clamps", d, h)
    st, gr, pt = T.substep(inp, h, T.DT, sc["params"].gravity)
    cells, mv = _grid(st32)
    assert not _fails_grid(gr, cells, mv)
    bad = T.Grid(inp, st, T.DT, sc["params"].gravity, variant=("grid_clamp_inv_dt",))
    assert _fails_grid(gr, cells, _moved(mv, gr, bad, cells, d))


def _moved(mv, gr, bad, cells, d):
    """the fp32 grid moved by (mutated truth - truth) at every node"""
    i = gr.lookup(cells)
    out = mv.copy()
    ok = i >= 0
    out[ok, :d] += (bad.vel - gr.vel)[i[ok]]
    return out
