"""The force-field rule of include/wgsparkl_hip_forces.h (wgs_set_force_fields) in numpy, fp64, from fp32 node values, and the truth
substep with fields: transfer_truth.Grid, then the fields, then wall_truth.apply, then transfer_truth.Particles. Shared by
tests/test_force_truth.py (CPU: the properties of the rule, the bounds against an fp32 restatement, mistakes that must be caught) and
tests/test_gpu_forces.py (the HIP kernel node by node, the fused G2P particle by particle).

A field is a wgsparkl_amd.models.ForceField (or anything with its attributes), or None for an entry that is skipped; `fields` holds up
to eight of them and they apply in that order, each on the running value, to the nodes with mass > 0 inside its region. What the
device reads is fp32: every parameter is rounded to fp32 first (`Field`), the axis of a 3D vortex is normalised in double and rounded
once, h and dt are the fp32 h and dt. The node position is x = cell * h (the device rounds that product: part of e_x below).

The bounds, by counting roundings (C_GU's style; u = 2^-24, D = dimension, p = falloff). Per accelerating field at a node, with v the
running value, a the acceleration, r the vector the rule takes from x (center - x, or x - center):

  - An input error e passes unchanged: the acceleration does not depend on v.
  - The position error is e_x = u (|x| + |r|): x = fl(cell h) is within u |x| of cell h, r = fl(center - x) within u |r| of its exact
    difference. A 3D VORTEX projects r onto the plane of its axis as well: r.n (three products, two additions), its product with n and
    the subtraction are six roundings of values no larger than |r|, so e_x grows by C_PROJ u |r|, C_PROJ = 6 (|r|, not |rp|: a node
    close to the axis and far along it is where the projection cancels).
  - The rule's Lipschitz constant in x is at most (1 + p) |strength| w_p(q): |d(w_p r)/dr| <= (1 + p) w_p, since q >= |r|^2.
  - What is left is relative to the terms themselves. q = softening^2 + sum r_k^2 is D + 1 products and D additions of non-negative
    numbers: (D + 2) u relative. w_p(q): a correctly rounded root halves that and adds u, every quotient adds u: at most 1.5 (D + 2) u
    + 3 u = 10.5 u (p = 3, D = 3). n x rp: two products and a difference per component, 3 u |rp| normwise. c = dt strength w_p: 2 u.
    c t + v: one rounding of the product (none when fused) and one of the sum: u dt |a| + u (|v| + dt |a|). Together at most
    17.5 u dt |a| + u |v|; C_FORCE = 24 leaves room for the second-order terms and for either evaluation order.
  So the added error is dt (1 + p) |strength| w_p(q) e_x + C_FORCE u (|v| + dt |a|).

DRAG is 1-Lipschitz in v (0 <= s <= 1: v' = (1 - s) v + s vec), so an input error does not grow. kdt = fl(strength dt), 1 + kdt and the
quotient: s within 3 u s; 1 - s another u; the two products and the sum (one of the products fused or not) 2 u (|v| + |vec|): at most
6 u (|v| + |vec|), C_DRAG = 8.

Region membership is decided in fp32 on the device, so a truth that relies on it must not be ambiguous: `ambiguous` counts the nodes
that lie within the position error of a region face (BOX: per axis, u (|x_k| + |x_k - c_k|) + u half_k) or of its sphere (BALL: the
distance |x - c| against the radius, within e_x + 4 u radius — the squares, their sum and radius^2 are D + 2 more roundings of values
near radius^2, half of that in the distance). The cap is 0 nodes; faces at (k + 1/2) h are h / 2 from every node."""
from __future__ import annotations

import numpy as np

import transfer_truth as T
import wall_truth as W

NONE, UNIFORM, RADIAL, VORTEX, DRAG = 0, 1, 2, 3, 4
ALL, BOX, BALL = 0, 1, 2
C_FORCE = 24.0    # rounding of one accelerating field, in units of u (|v| + dt |a|)
C_DRAG = 8.0      # rounding of one drag field, in units of u (|v| + |vec|)
C_PROJ = 6.0      # the projection of a 3D vortex, in units of u |r|, added to the position error
VARIANTS = ("radial_x_minus_center", "no_softening", "reverse_order", "massless_forced", "drag_explicit")   # mistakes `apply` can make on request


def f32(x):
    return np.asarray(np.asarray(x, np.float32), np.float64)


class Field:
    """one field as the device reads it: fp32 parameters (as fp64 numbers), d components, the vortex axis normalised"""

    def __init__(self, f, d):
        self.kind, self.p, self.region = int(f.kind), int(f.falloff), int(f.region)
        self.strength, self.soft = float(f32(f.strength)), float(f32(f.softening))
        v3 = lambda a: f32((tuple(a) + (0.0, 0.0, 0.0))[:3])
        self.center, self.rc, self.rh = v3(f.center)[:d], v3(f.region_center)[:d], v3(f.region_half)[:d]
        vec = v3(f.vec)
        if self.kind == VORTEX and d == 3:
            vec = f32(vec / np.sqrt((vec * vec).sum()))
        self.vec = vec[:d]
        self.radius = float(v3(f.region_half)[0])


def fields_of(fields, d):
    return [None if f is None or int(f.kind) == NONE else Field(f, d) for f in fields]


def positions(cells, h):
    return np.asarray(cells, np.float64) * float(np.float32(h))


def weight(p, q):
    return (np.ones_like(q), 1.0 / np.sqrt(q), 1.0 / q, 1.0 / (q * np.sqrt(q)))[p]


def inside(x, f: Field):
    """membership of positions [M, d] in the region of f"""
    if f.region == ALL:
        return np.ones(len(x), bool)
    if f.region == BOX:
        return np.all(np.abs(x - f.rc) <= f.rh, axis=1)
    return ((x - f.rc) ** 2).sum(1) <= f.radius ** 2


def members(cells, h, fields):
    """[M, len(fields)] bool: which fields' regions each node is in (whatever its mass; False for a skipped entry)"""
    cells = np.asarray(cells)
    x = positions(cells, h)
    out = np.zeros((len(cells), len(fields)), bool)
    for i, f in enumerate(fields_of(fields, cells.shape[1])):
        if f is not None:
            out[:, i] = inside(x, f)
    return out


def ambiguous(cells, h, fields, u=T.U32):
    """[M] bool: the nodes whose membership in some region an fp32 evaluation may decide the other way (see the module docstring)"""
    cells = np.asarray(cells)
    x = positions(cells, h)
    out = np.zeros(len(cells), bool)
    for f in fields_of(fields, cells.shape[1]):
        if f is None or f.region == ALL:
            continue
        r = x - f.rc
        if f.region == BOX:
            out |= np.any(np.abs(np.abs(r) - f.rh) <= u * (np.abs(x) + np.abs(r) + f.rh), axis=1)
        else:
            dist = np.linalg.norm(r, axis=1)
            e_x = u * (np.linalg.norm(x, axis=1) + dist)
            out |= np.abs(dist - f.radius) <= e_x + 4.0 * u * f.radius
            # the bounding box the kernel also asks for: |r_k| <= radius is implied unless it is within rounding of it
            out |= np.any((np.abs(r) > f.radius) & (np.abs(r) - f.radius <= u * (np.abs(x) + np.abs(r) + f.radius)), axis=1)
    return out


def _accel(f: Field, x, variant=()):
    """(acceleration a [M, d], Lipschitz constant in x [M], position error scale |x| + (1 + C) |r| [M]) of an accelerating field"""
    d = x.shape[1]
    if f.kind == UNIFORM:
        return np.broadcast_to(f.vec, x.shape).copy(), np.zeros(len(x)), np.zeros(len(x))
    soft2 = 0.0 if "no_softening" in variant else f.soft ** 2
    if f.kind == RADIAL:
        r = x - f.center if "radial_x_minus_center" in variant else f.center - x
        q = (r * r).sum(1) + soft2
        t, proj = r, 0.0
    else:
        r = x - f.center
        if d == 2:
            rp, t, proj = r, np.stack([-r[:, 1], r[:, 0]], 1), 0.0
        else:
            rp = r - (r @ f.vec)[:, None] * f.vec[None, :]
            t, proj = np.cross(np.broadcast_to(f.vec, rp.shape), rp), C_PROJ
        q = (rp * rp).sum(1) + soft2
    with np.errstate(divide="ignore", invalid="ignore"):
        w = weight(f.p, q)
    rn = np.linalg.norm(r, axis=1)
    return f.strength * w[:, None] * t, (1.0 + f.p) * abs(f.strength) * w, np.linalg.norm(x, axis=1) + (1.0 + proj) * rn


def _drag_s(f: Field, dt):
    kdt = min(f.strength * dt, 1e30)
    return kdt / (1.0 + kdt)


def _run(cells, vel, mass, h, dt, fields, bound_in=None, u=T.U32, variant=()):
    cells = np.asarray(cells)
    d = cells.shape[1]
    x = positions(cells, h)
    dt = float(np.float32(dt))
    v = np.array(vel, np.float64)
    b = np.zeros(len(v)) if bound_in is None else np.array(bound_in, np.float64)
    massy = np.ones(len(v), bool) if "massless_forced" in variant else np.asarray(mass, np.float64) > 0.0
    fs = fields_of(fields, d)
    for f in (fs[::-1] if "reverse_order" in variant else fs):
        if f is None:
            continue
        sel = inside(x, f) & massy
        vn = np.linalg.norm(v, axis=1)
        if f.kind == DRAG:
            s = _drag_s(f, dt)
            new = v + min(f.strength * dt, 1e30) * (f.vec - v) if "drag_explicit" in variant else (1.0 - s) * v + s * f.vec
            add = C_DRAG * u * (vn + np.linalg.norm(f.vec))
        else:
            a, lip, xs = _accel(f, x, variant)
            new = v + dt * a
            add = dt * lip * u * xs + C_FORCE * u * (vn + dt * np.linalg.norm(a, axis=1))
        v = np.where(sel[:, None], new, v)
        b = np.where(sel, b + add, b)
    return v, b


def apply(cells, vel, mass, h, dt, fields, variant=()):
    """the rule on node velocities [M, d] (fp32 or fp64 values, computed in fp64) of masses [M] at world cells [M, d]; returns fp64
    [M, d]. `variant`: one of VARIANTS, a mistake made on purpose (tests/test_force_truth.py shows that the bounds catch it)."""
    return _run(cells, vel, mass, h, dt, fields, variant=variant)[0]


def node_bound(cells, vel_in, mass, h, dt, fields, bound_in=None, u=T.U32):
    """bound [M] of the forced node velocities of a kernel of unit roundoff u whose inputs carry `bound_in` (the module docstring)"""
    return _run(cells, vel_in, mass, h, dt, fields, bound_in=bound_in, u=u)[1]


def substep(inp: T.Inputs, h, dt, gravity, fields, walls=None, u=T.U32, extra_levels=0.0):
    """(Stencil, Grid, forced [and walled] node velocities [M, d], their bounds [M], Particles) of the fp64 substep with fields: the
    end-to-end truth. Asserts that no node's region membership is ambiguous."""
    st = T.Stencil(inp, h)
    gr = T.Grid(inp, st, dt, gravity)
    assert not ambiguous(gr.cells, h, fields, u).any(), "a node lies within rounding of a region face"
    _, bv, _ = gr.bounds(u, extra_levels)
    vf, bf = _run(gr.cells, gr.vel, gr.mass, h, dt, fields, bound_in=bv, u=u)
    if walls is not None:
        bf = W.node_bound(gr.cells, vf, walls, bf, u)
        vf = W.apply(gr.cells, vf, walls)
    pt = T.Particles(inp, st, vf[gr.inv], dt, node_bound=bf[gr.inv], u=u)
    return st, gr, vf, bf, pt


# ------------------------------------------------------------------------------------------------ scenes
# What tests/test_gpu_forces.py runs and tests/test_force_truth.py checks from the truth alone. Region faces lie at (k + 1/2) h, chosen
# so that the kernel's wave-uniform reject can go wrong in every way it can: between a block's last node and the next block's first
# (3D, blocks of 4: cells 3|4 and 7|8; 2D, blocks of 8: 7|8 and 15|16), in the middle of a block, at a negative coordinate, and a
# ball whose bounding box reaches a block (its node 8 alone) that the ball itself does not.
CASES = [(2, 1.0), (2, 0.3), (3, 0.3), (3, 1.0)]
EXTENT = {2: (-10, 26), 3: (-8, 14)}                              # the cloud, in cells
BOX_FACES = {3: [(-2.5, 3.5), (1.5, 7.5), (-4.5, 9.5)], 2: [(-3.5, 7.5), (3.5, 15.5)]}   # (low, high) per axis, in cells
BALL = {3: ((5.5, 5.5, 5.5), 3.7), 2: ((3.5, 3.5), 5.2)}          # (centre, radius) in cells: a whole block inside, a box corner block outside
CENTER = {3: (5.3, 2.1, 4.4), 2: (6.2, 9.7)}                      # of the radial and vortex fields, in cells: off every node
AXIS = (0.3, 1.0, -0.4)                                           # of the 3D vortex: oblique
KINDS = [("uniform", 0), ("drag", 0)] + [(k, p) for k in ("radial", "vortex") for p in range(4)]
REGIONS = ("all", "box", "ball")


def cloud(d, h, seed=0, n=None, vel_scale=6.0):
    """a cloud over EXTENT[d]: coordinates on both sides of 0, blocks wholly inside, wholly outside and cut by every region"""
    rng = np.random.default_rng(300 * d + seed)
    lo, hi = EXTENT[d]
    return T._finish(rng.uniform(lo * h, hi * h, (n or (9000 if d == 3 else 3000), d)), h, rng, vel_scale=vel_scale * h)


def in_region(f, d, h, region):
    """the field `f` confined to the scenes' box or ball (`region`: one of REGIONS)"""
    if region == "box":
        faces = np.array(BOX_FACES[d], np.float64) * h
        return f.within_box(tuple(faces.mean(1)), tuple(0.5 * (faces[:, 1] - faces[:, 0])))
    if region == "ball":
        c, r = BALL[d]
        return f.within_ball(tuple(np.array(c) * h), r * h)
    return f


def field(kind, p, d, h, region="all", sign=1.0):
    """a field of the scenes: strengths that move a node by a few tenths of h per substep at dt = 1e-3, softening 1.5 h"""
    from wgsparkl_amd.models import ForceField
    c = tuple(np.array(CENTER[d]) * h)
    if kind == "uniform":
        f = ForceField.uniform(tuple(np.array([300.0, -450.0, 200.0][:d]) * h * sign))
    elif kind == "drag":
        f = ForceField.drag(700.0, tuple(np.array([4.0, -3.0, 2.5][:d]) * h * sign))
    else:
        strength = sign * (50.0, 500.0 * h, 5000.0 * h * h, 5.0e4 * h ** 3)[p]
        f = ForceField.radial(c, strength, p, 1.5 * h) if kind == "radial" else ForceField.vortex(c, strength, AXIS, p, 1.5 * h)
    return in_region(f, d, h, region)


def eight(d, h):
    """eight overlapping fields with a NONE among them (what the GPU test of the maximum sets)"""
    return [field("uniform", 0, d, h, "box"), field("radial", 1, d, h, "all"), None, field("vortex", 2, d, h, "ball"),
            field("drag", 0, d, h, "box"), field("radial", 3, d, h, "ball", sign=-1.0), field("vortex", 0, d, h, "all"),
            field("uniform", 0, d, h, "all", sign=-0.5)]


def block_classes(cells, h, f, d):
    """(blocks wholly inside, wholly outside, cut) by the region of field `f`, counted over the 64-node blocks of `cells`; and how many
    blocks the region's bounding box reaches although none of their nodes is inside (a ball's box corners)"""
    cells = np.asarray(cells)
    bw = T.bw_of(d)
    fl = Field(f, d)
    x = positions(cells, h)
    ins = inside(x, fl)
    half = fl.rh if fl.region == BOX else np.full(d, fl.radius)
    in_box = np.all(np.abs(x - fl.rc) <= half, axis=1) if fl.region != ALL else np.ones(len(x), bool)
    _, inv = np.unique(T.node_key(cells // bw), return_inverse=True)
    inv = inv.reshape(-1)
    tot = np.bincount(inv)
    n_in, n_box = np.bincount(inv, ins.astype(np.float64)), np.bincount(inv, in_box.astype(np.float64))
    full = tot == 64
    return int((full & (n_in == 64)).sum()), int((full & (n_in == 0)).sum()), int((full & (n_in > 0) & (n_in < 64)).sum()), int(((n_box > 0) & (n_in == 0)).sum())
