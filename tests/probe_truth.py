"""fp64 truth of a grid sample (include/wgsparkl_hip.h "Eulerian field output") from a grid given as (cells, vel_mass) — what
MpmData.read_grid() returns —, with its bounds, the point sets the checks use, and the dense window of such a grid. Shared by
tests/test_probe_truth.py (CPU: the truth against transfer_truth.isolated, an fp32 numpy evaluation in both summation orders
inside the bounds) and tests/test_gpu_probe.py (the HIP sampler record by record).

A sample is a G2P at a foreign point: the truth is transfer_truth.Particles on a transfer_truth.Stencil whose positions are the
probe points, with the node values of the given grid and ZERO for every stencil node the grid does not hold (isolated() asserts
there instead). Bounds: velocity and gradient are Particles.b_vel_g / b_grad as they stand; the density takes the form of
b_vel_g with m_i in the place of |v_i| — C_G2P u sum w m + C_WT u weight_error sum m, over h^D — plus C_UPD u density for the
division by h^D. No constant of its own.

One term comes from the number format, not from a constant: the relative model fl(a op b) = (a op b)(1 + delta) does not hold where a
result is subnormal, and node masses ARE subnormal in these scenes (a particle one ulp off a tie on every axis leaves ~1e-42 of its
mass on a node). There every rounded operation errs by up to half the spacing of the subnormals (2^-150 in fp32) absolutely, so the
density bound adds that for the at most 3 * 3^D rounded operations on the mass path of either summation order (weights are <= 1 and
do not amplify it), over h^D, and once more for the division. Velocities are not subnormal: their bounds stand as they are."""
import numpy as np

import transfer_truth as T
from oracle.np_oracle import assoc_cell, block_cells, bw_of, shifts_of

SUBNORMAL_SPACING = {T.U32: 2.0 ** -149, T.U64: 2.0 ** -1074}
MAX_CELLS = 2.0 ** 22     # |x / h| at or beyond this is outside every key range: decided on the floats


def key_range_ok(blocks, d):
    """block_in_key_range (device_math.h) of block coordinates [..., d]"""
    b = np.asarray(blocks, np.int64)
    if d == 2:
        ok = np.all((b >= -0x7fff) & (b <= 0x8000), axis=-1)
        return ok & ~((b[..., 0] >= 0x7fff) & (b[..., 1] == 0x8000))
    lo = np.array([-0x3ff, -0x1ff, -0x3ff])
    hi = np.array([0x400, 0x200, 0x400])
    ok = np.all((b >= lo) & (b <= hi), axis=-1)
    return ok & ~((b[..., 0] >= 0x3ff) & (b[..., 1] == 0x200) & (b[..., 2] == 0x400))


def bad_points(points, h):
    """a non-finite coordinate, or a stencil that reaches a block outside the packed key range: an all-zero record"""
    p = np.asarray(points, np.float32)
    d = p.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        far = ~np.isfinite(p).all(1) | ~(np.abs(p.astype(np.float64)) / float(np.float32(h)) < MAX_CELLS).all(1)
    safe = np.where(far[:, None], np.float32(0), p)
    cell = assoc_cell(safe, h)
    bw = bw_of(d)
    b0, b1 = cell // bw, (cell + 2) // bw
    ok = np.ones(len(p), bool)
    for o in range(1 << d):
        sel = np.array([(o >> k) & 1 for k in range(d)], bool)
        ok &= key_range_ok(np.where(sel[None, :], b1, b0), d)
    return far | ~ok


def _dummy_inputs(points32):
    n, d = points32.shape
    z = np.zeros
    return T.Inputs(points32, z((n, d)), z((n, d * d)), z((n, d * d)), z(n), z(n), z(n), z(n))


def _gather(st, d, cells, vel_mass):
    """node values [n, S, d + 1] (0 where absent) and presence [n, S] of every stencil node"""
    n, S = st.node.shape[:2]
    vm = np.asarray(vel_mass, np.float64)
    if len(cells) == 0:
        return np.zeros((n, S, d + 1)), np.zeros((n, S), bool)
    keys = T.node_key(cells)
    order = np.argsort(keys)
    sk = keys[order]
    want = T.node_key(st.node.reshape(-1, d))
    i = np.minimum(np.searchsorted(sk, want), len(sk) - 1)
    present = sk[i] == want
    val = np.where(present[:, None], vm[order][i], 0.0)
    return val.reshape(n, S, d + 1), present.reshape(n, S)


class Truth:
    """velocity [n, d], gradient [n, row, col], density [n], active_nodes [n] and the bounds b_vel, b_grad, b_dens [n]"""

    def __init__(self, points, h, cells, vel_mass, u=T.U32):
        p = np.ascontiguousarray(points, np.float32)
        n, d = p.shape
        self.d, self.h = d, float(h)
        self.bad = bad_points(p, h)
        safe = np.where(self.bad[:, None], np.float32(0), p)
        inp = _dummy_inputs(safe)
        st = T.Stencil(inp, h)
        val, present = _gather(st, d, cells, vel_mass)
        val[self.bad] = 0.0
        present[self.bad] = False
        pt = T.Particles(inp, st, val[..., :d], T.DT, u=u)
        m = val[..., d]
        hd = self.h ** d
        self.velocity, self.gradient = pt.vel_g, pt.grad
        self.density = np.einsum("ns,ns->n", st.w, m) / hd
        self.active_nodes = present.sum(1).astype(np.uint32)
        self.b_vel, self.b_grad = pt.b_vel_g, pt.b_grad
        self.b_dens = (T.C_G2P * u * np.einsum("ns,ns->n", st.w, np.abs(m)) + T.C_WT * u * st.weight_error * np.abs(m).sum(1)) / hd + \
            T.C_UPD * u * np.abs(self.density) + 0.5 * SUBNORMAL_SPACING[u] * (3.0 * 3 ** d / hd + 1.0)
        self.stencil, self.inputs, self.node_values = st, inp, val


def compare(tag, truth, velocity, gradient, density, active_nodes, fails, sel=None):
    """every record against the truth: the three bounded fields through transfer_truth.check (margins reported), active_nodes and the
    all-zero records of bad points exactly"""
    v = np.asarray(velocity, np.float64)
    g = np.asarray(gradient, np.float64)
    r = np.asarray(density, np.float64)
    a = np.asarray(active_nodes)
    if not (np.isfinite(v).all() and np.isfinite(g).all() and np.isfinite(r).all()):
        fails.append(f"{tag}: non-finite values in a record")
        return
    T.check(f"{tag}: sample velocity (scale sum w |v_i|)", np.linalg.norm(v - truth.velocity, axis=1), truth.b_vel, fails, sel)
    T.check(f"{tag}: sample gradient (scale sum w |v_i| |dpt| 4 / h^2)", np.linalg.norm(g - truth.gradient, axis=(1, 2)), truth.b_grad, fails, sel)
    T.check(f"{tag}: sample density (scale sum w m / h^D)", np.abs(r - truth.density), truth.b_dens, fails, sel)
    s = np.ones(len(a), bool) if sel is None else np.asarray(sel)
    wrong = s & (a != truth.active_nodes)
    if wrong.any():
        i = int(np.argmax(wrong))
        fails.append(f"{tag}: active_nodes differs at {int(wrong.sum())} points (first #{i}: {int(a[i])} != {int(truth.active_nodes[i])})")
    z = s & truth.bad
    if z.any() and (np.abs(v[z]).max() != 0 or np.abs(g[z]).max() != 0 or np.abs(r[z]).max() != 0 or a[z].max() != 0):
        fails.append(f"{tag}: a bad point's record is not all zero")


# ------------------------------------------------------------------------------------------------ fp32 evaluations (numpy)
def eval32(points, h, cells, vel_mass, order):
    """The three formulas in fp32, every operation rounded, in one of two summation orders: "direct" = the 3^D terms one after the
    other (x fastest), "tensor" = the tensor-product order of the step's G2P (x, then y, then z). The grid is rounded to fp32.
    Returns velocity [n, d], gradient [n, row, col], density [n], active_nodes [n]."""
    f = np.float32
    p = np.ascontiguousarray(points, f)
    n, d = p.shape
    bad = bad_points(p, h)
    safe = np.where(bad[:, None], f(0), p)
    h32 = f(h)
    inv_h = f(1.0) / h32
    invd = f(4.0) / (h32 * h32)
    cell = assoc_cell(safe, h)
    ref = cell.astype(f) * h32 - safe                                  # [n, d]
    t = -ref * inv_h
    w = np.stack([f(0.5) * (f(1.5) - t) * (f(1.5) - t), f(0.75) - (t - f(1.0)) * (t - f(1.0)), f(0.5) * (t - f(0.5)) * (t - f(0.5))], -1)   # [n, d, 3]
    st = T.Stencil(_dummy_inputs(safe), h)                             # (only its node list is used)
    val, present = _gather(st, d, cells, np.asarray(vel_mass, f))
    val = val.astype(f)
    val[bad] = 0
    present[bad] = False
    sh = shifts_of(d)
    vel = np.zeros((n, d), f)
    grad = np.zeros((n, d, d), f)
    dens = np.zeros(n, f)
    if order == "direct":
        for s, off in enumerate(sh):
            wt = w[:, 0, off[0]] * w[:, 1, off[1]]
            if d == 3:
                wt = wt * w[:, 2, off[2]]
            dpt = ref + off.astype(f)[None, :] * h32
            wv = wt[:, None] * val[:, s, :d]
            vel = vel + wv
            grad = grad + wv[:, :, None] * dpt[:, None, :]
            dens = dens + wt * val[:, s, d]
        grad = invd * grad
    else:
        G = np.zeros((n, d, d), f)                                     # G[:, c, r]
        acc = np.zeros((n, d + 1), f)
        S = val.reshape((n,) + (3,) * d + (d + 1,))                    # [n, sx, sy(, sz), comp]
        for sz in range(3 if d == 3 else 1):
            Pz = np.zeros((n, d + 1), f)
            Gxz = np.zeros((n, d), f)
            Gyz = np.zeros((n, d), f)
            for sy in range(3):
                a = [S[:, sx, sy, sz] if d == 3 else S[:, sx, sy] for sx in range(3)]
                pr = w[:, 0, 0, None] * a[0] + w[:, 0, 1, None] * a[1] + w[:, 0, 2, None] * a[2]
                gx = w[:, 0, 1, None] * a[1][:, :d] + (f(2.0) * w[:, 0, 2])[:, None] * a[2][:, :d]
                wy = w[:, 1, sy, None]
                Pz = Pz + wy * pr
                Gxz = Gxz + wy * gx
                if sy:
                    Gyz = Gyz + (f(sy) * wy) * pr[:, :d]
            wz = w[:, 2, sz, None] if d == 3 else f(1.0)
            acc = acc + wz * Pz
            G[:, 0] = G[:, 0] + wz * Gxz
            G[:, 1] = G[:, 1] + wz * Gyz
            if d == 3:
                G[:, 2] = G[:, 2] + (f(sz) * wz) * Pz[:, :d]
        vel, dens = acc[:, :d], acc[:, d]
        grad = invd * (vel[:, :, None] * ref[:, None, :] + h32 * G.transpose(0, 2, 1))
    hd = h32 * h32 * (h32 if d == 3 else f(1.0))
    out_v, out_g, out_r = vel.copy(), grad.copy(), dens / hd
    out_v[bad], out_g[bad], out_r[bad] = 0, 0, 0
    return out_v, out_g, out_r, present.sum(1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ point sets, grids, windows
CASES = [(name, d, h) for name in ("coordinates", "ties") for d in (2, 3) for h in (0.3, 0.5)]


def tie_points(base, h, rng, count=60):
    """for each axis: points with x / h = k + 0.5 (exact where h is a power of two) and their one-ulp neighbours, the other
    coordinates taken from `base` [m, d]"""
    base = np.asarray(base, np.float32)
    d = base.shape[1]
    out = []
    for axis in range(d):
        rows = base[rng.integers(0, len(base), count)].copy()
        k = np.rint(rows[:, axis].astype(np.float64) / h)
        x = ((k + 0.5) * h).astype(np.float32)
        for v in (x, np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))):
            r = rows.copy()
            r[:, axis] = v
            out.append(r)
    return np.concatenate(out)


def probe_points(positions, h, cells, seed=0):
    """The point sets of the truth comparison, as (name, points fp32 [n, d]) pairs: the scene's own particle positions, those
    positions jittered by up to 1.5 h (stencils hang over the rim of the active set), every node position cell * h of the grid, and
    the ties of every axis with their one-ulp neighbours."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(positions, np.float32)
    d = pos.shape[1]
    jit = (pos.astype(np.float64) + rng.uniform(-1.5 * h, 1.5 * h, pos.shape)).astype(np.float32)
    nodes = (np.asarray(cells, np.float64) * h).astype(np.float32).reshape(-1, d)
    return [("own positions", pos), ("jittered by 1.5 h", jit), ("node positions", nodes), ("ties", tie_points(pos, h, rng))]


def whole_block_grid(gr):
    """(cells, vel_mass fp32) of every node of every block that holds a node of the fp64 transfer_truth.Grid `gr`: what a read-back
    grid looks like (whole blocks, zeros where no particle reaches)"""
    d = gr.d
    blocks = np.unique(gr.cells // bw_of(d), axis=0)
    cells = block_cells(blocks, d)
    i = gr.lookup(cells)
    vm = np.zeros((len(cells), d + 1), np.float32)
    ok = i >= 0
    vm[ok, :d] = gr.vel[i[ok]]
    vm[ok, d] = gr.mass[i[ok]]
    return cells, vm


def dense_window(cells, vel_mass, lo, dims):
    """read_grid()'s (cells, vel_mass) scattered into (velocity [dims..., d], mass [dims...]) fp32 arrays of the window lo, dims;
    +0 where the grid holds no node"""
    lo = np.asarray(lo, np.int64)
    dims = tuple(int(x) for x in dims)
    d = len(dims)
    vel = np.zeros(dims + (d,), np.float32)
    mass = np.zeros(dims, np.float32)
    if len(cells):
        rel = np.asarray(cells, np.int64) - lo[None, :]
        inside = np.all((rel >= 0) & (rel < np.array(dims)[None, :]), axis=1)
        idx = tuple(rel[inside].T)
        vm = np.asarray(vel_mass, np.float32)
        vel[idx] = vm[inside, :d]
        mass[idx] = vm[inside, d]
    return vel, mass
