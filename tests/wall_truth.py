"""The domain-wall rule of include/wgsparkl_hip.h (wgs_set_domain_walls) in numpy, fp64, from fp32 node values, and the truth
substep with walls: transfer_truth.Grid, then the rule, then transfer_truth.Particles. Shared by tests/test_wall_truth.py (CPU: the
properties of the rule) and tests/test_gpu_walls.py (the HIP kernel node by node, the fused G2P particle by particle).

A face is (type, friction, plane) — a wgsparkl_amd.models.Wall or a triple — or None; `walls` holds 2 * d of them, walls[2 k] the
low face of axis k (nodes with cell[k] <= plane), walls[2 k + 1] its high face (cell[k] >= plane). A node inside several faces
takes them in that order on the running value.

Where friction == 0 the rule only ever writes +0 or keeps a value, so its fp64 result from fp32 inputs IS an fp32 array, bit for
bit (`bits`). With friction the rule is a sum of at most two squares, a root, a quotient, a product, a difference and a product:
C_WALL u |v| normwise per frictional face. The rule is 1-Lipschitz in vt and friction-Lipschitz in vn (projection and
soft-thresholding), so an input error e becomes at most (1 + friction) e per frictional face (`lipschitz`)."""
from __future__ import annotations

import numpy as np

import transfer_truth as T

NONE, STICKY, SLIP, SEPARATE = 0, 1, 2, 3
C_WALL = 8.0      # rounding of one frictional face, in units of u |v| (C_GU's style of count)


def face(w):
    """(type, friction, plane) of a face, or None for no face"""
    if w is None:
        return None
    t, fr, pl = (w.type, w.friction, w.plane) if hasattr(w, "plane") else w
    return None if int(t) == NONE else (int(t), float(fr), int(pl))


def inside(cells, f, plane):
    """membership of world cells [M, d] in face f (2 k + side) at `plane`"""
    c = np.asarray(cells)[:, f >> 1]
    return c >= plane if f & 1 else c <= plane


def members(cells, walls):
    """[M, 2 d] bool: which faces each node is in"""
    cells = np.asarray(cells)
    out = np.zeros((len(cells), len(walls)), bool)
    for f, w in enumerate(walls):
        w = face(w)
        if w is not None:
            out[:, f] = inside(cells, f, w[2])
    return out


def apply(cells, vel, walls):
    """the rule on node velocities [M, d] (fp32 or fp64 values, computed in fp64) at world cells [M, d]; returns fp64 [M, d]"""
    v = np.array(vel, np.float64)
    d = v.shape[1]
    assert len(walls) == 2 * d
    for f, w in enumerate(walls):
        w = face(w)
        if w is None:
            continue
        typ, fr, plane = w
        k = f >> 1
        ins = inside(cells, f, plane)
        vn = v[:, k].copy() if f & 1 else -v[:, k]
        if typ == STICKY:
            v[ins] = 0.0
            continue
        act = ins & (vn > 0.0) if typ == SEPARATE else ins
        v[act, k] = 0.0
        if fr > 0.0:
            others = [j for j in range(d) if j != k]
            vt = np.sqrt((v[:, others] ** 2).sum(1))
            sel = act & (vt > 0.0)
            s = np.maximum(0.0, 1.0 - fr * np.abs(vn[sel]) / vt[sel])
            for j in others:
                v[sel, j] *= s
    return v


def bits(a):
    """the fp32 bit patterns of an array (values that are fp32 numbers)"""
    a32 = np.asarray(a, np.float32)
    assert np.array_equal(a32.astype(np.float64), np.asarray(a, np.float64), equal_nan=True), "not an fp32 array"
    return np.ascontiguousarray(a32).view(np.uint32)


def lipschitz(cells, walls):
    """per node: (product over the faces it is in of (1 + friction), number of those faces with friction > 0)"""
    m = members(cells, walls)
    L = np.ones(len(m))
    nf = np.zeros(len(m))
    for f, w in enumerate(walls):
        w = face(w)
        if w is not None and w[0] != STICKY and w[1] > 0.0:
            L = np.where(m[:, f], L * (1.0 + w[1]), L)
            nf += m[:, f]
    return L, nf


def node_bound(cells, vel_in, walls, bound_in, u=T.U32):
    """bound of the walled node velocities of a kernel of unit roundoff u whose inputs carry `bound_in`: (1 + friction) bound_in +
    C_WALL u |v| per frictional face the node is in (one such face: the formula as it stands)"""
    L, nf = lipschitz(cells, walls)
    return L * np.asarray(bound_in, np.float64) + C_WALL * u * nf * np.linalg.norm(np.asarray(vel_in, np.float64), axis=1)


def substep(inp: T.Inputs, h, dt, gravity, walls, u=T.U32):
    """(Stencil, Grid, walled node velocities [M, d], their bounds [M], Particles) of the fp64 substep with walls: the end-to-end truth"""
    st = T.Stencil(inp, h)
    gr = T.Grid(inp, st, dt, gravity)
    _, bv, _ = gr.bounds(u)
    vw = apply(gr.cells, gr.vel, walls)
    bw = node_bound(gr.cells, gr.vel, walls, bv, u)
    pt = T.Particles(inp, st, vw[gr.inv], dt, node_bound=bw[gr.inv], u=u)
    return st, gr, vw, bw, pt
