"""fp64 truth of the CPIC colour distance field of analytic colliders (ball, cuboid, capsule): the node field from closed
forms of the signed distance, the particle field (g2p_cdf.wgsl:39-250) from a given node field, per-element rounding
bounds, the sets of elements an fp32 evaluation may decide either way, and the scenes. truth_of builds the Truth (rigid,
nodes, particles) of any scene: with mesh colliders tests/mesh_truth.py fills their columns of the node field, without one
`rigid` is None. The comparisons with the C oracle (_oracle_fields, assert_matches_fp64_oracle,
assert_fp32_oracle_fits_and_caps_hold) are shared by tests/test_cdf_truth.py and tests/test_mesh_truth.py (CPU: the truth
against the C fp64 oracle, the bounds against the C fp32 oracle, perturbations); tests/test_gpu_cdf.py and
tests/test_gpu_mesh_cdf.py check the HIP kernels node by node and particle by particle (gpu_common.checked_substep).

Inputs are the values the library receives: fp32 positions, fp32 collider parameters (the scenes round every collider
parameter to fp32, the 2D rotation is (cos, sin) of the fp32 angle in fp32), h as the Python float (the kernel's fp32 h
is one of the roundings the bounds count). The closed forms are a second derivation: they are written from the geometry
(|p| - r, distance to a segment minus r, the box distance with the face of least penetration inside), evaluated in the
collider's frame, and mapped back with the pose. The pose maps use the rotation the parameters define (the matrix of the
quaternion / of (cos, sin) as given, its transpose as the inverse), so that a rotation that is a unit one only to fp32
does not separate the truth from an fp64 evaluation of the same parameters.

Bounds are fixed multiples of u = 2^-24 times stated scales (tests/transfer_truth.py's convention); the multiples are
settled against the C fp32 oracle in tests/test_cdf_truth.py, never against the kernels."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

import transfer_truth as T
from helpers import oracle, report_margin
from oracle.np_oracle import assoc_cell, block_cells, eval_all

U32 = T.U32
NONE = 0xFFFFFFFF
NO_VOTER = 1.0e10
MAXC = 16

# ---- fixed multiples of u
# Node distance of one collider: b = u (C_FAR (|pt| + |trans|) + C_NEAR[d] (|pt - trans| + scale extent)).
# C_FAR counts the roundings whose operands have the magnitude of the world coordinates: pt = cell * h (the fp32 h and
# the product: 2), pt - trans (1), rotated + trans (1), proj - pt (1) = 5.
# C_NEAR counts those whose operands have the magnitude of the collider and its distance to the node:
#   pose_to_local: 3D quat_rotate 2 products + difference (3) for t, w t + sum (2), u x t (3), sum (1) = 9, 2D 2 products +
#   sum = 3; the division by scale 1;  projection: ball / capsule D products + D - 1 sums + sqrt + r / n + product <= 8,
#   cuboid 3;  pose_to_world: the product by scale 1, the rotation 9 (3);  3D: 9 + 1 + 8 + 1 + 9 = 28, 2D: 3 + 1 + 7 + 1 + 3 =
#   15; a sum of D components is rounded at up to sqrt(D) times the norm of the vector: 28 sqrt(3) = 48, 15 sqrt(2) = 21.
C_FAR = 5.0
C_NEAR = {2: 21.0, 3: 48.0}
C_DIST = 4.0      # |proj - pt|: D products, D - 1 sums, sqrt, relative to the distance
# Particle field.
# vote: 3^D terms, each two products and a sum into one accumulator: (3^D + 3) u sum w |d|
# least squares: every entry of the Gram matrix and the right-hand side is such a sum (C_ACC = 3^D + 3), the LDL^T solve of
# D + 1 unknowns adds (D + 1)^2 multiply-subtracts in the factorisation and as many in the two substitutions (C_SOLVE)
C_VOTE = {2: 12.0, 3: 30.0}
C_ACC = {2: 9 + 3.0, 3: 27 + 3.0}
C_SOLVE = {2: 2 * 9.0, 3: 2 * 16.0}
C_ABS_T = 4.0     # t = -(cell h - x) / h: difference, product by 1 / h, 1 / h itself, and eval_all's own roundings


def f32(x):
    """the fp32 value of x as a Python float / float64 array"""
    return np.asarray(np.asarray(x, np.float32), np.float64)


def rot_matrix(rot, d):
    """the map quat_rotate / the 2D (cos, sin) pair define, as a matrix (fp64, not re-normalised)"""
    if d == 2:
        cs, sn = float(rot[0]), float(rot[1])
        return np.array([[cs, -sn], [sn, cs]])
    x, y, z, w = (float(v) for v in rot)
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + 2.0 * w * K + 2.0 * (K @ K)


def colliders_of(colliders, d, poses=None):
    """[dict(shape_type, shape, R, trans, scale)] of the fp32 values the library holds; `poses` = read_body_poses()
    replaces rotation and translation (the poses a moving collider has before a substep)."""
    out = []
    for i, c in enumerate(colliders):
        if poses is not None:
            rot, tr = poses[i]["rotation"], poses[i]["translation"]
        elif d == 2:
            ang = np.float32(c.rotation[0])
            rot, tr = (float(np.cos(ang)), float(np.sin(ang))), c.translation
        else:
            rot, tr = f32(c.rotation), c.translation
        shape = np.zeros(4)
        shape[:len(c.shape)] = f32(c.shape)
        out.append(dict(shape_type=int(c.shape_type), shape=shape, R=rot_matrix(f32(rot), d), trans=f32(tr)[:d].copy(),
                        scale=float(np.float32(c.scale))))
        if getattr(c, "vertices", None) is not None:        # a mesh collider: its local fp32 vertices and primitives
            out[-1].update(vertices=f32(c.vertices).reshape(-1, d), indices=np.asarray(c.indices, np.int64).reshape(-1, d))
    return out


def _is_exact(c, d, h):
    """every operation of the kernel is exact for this collider: an axis-aligned unscaled cuboid whose translation and
    half extents are multiples of h / 64, h a power of two (nodes within 2^15 cells of it)"""
    if c["shape_type"] != 1 or not T._pow2(h) or c["scale"] != 1.0 or not np.array_equal(c["R"], np.eye(d)):
        return False
    q = np.concatenate([c["trans"], c["shape"][:d]]) * (64.0 / h)
    return bool(np.all(q == np.rint(q)) and np.all(np.abs(q) < 2 ** 21))


# ------------------------------------------------------------------------------------------------ node field
def _project(c, pl, d, variant):
    """closest boundary point and signed distance in the collider's frame (pl [M, d]); `amp` = how much an error of pl
    tangent to the boundary is magnified in the projection (r / n for round shapes, 1 for flat faces)"""
    st, sh = c["shape_type"], c["shape"]
    M = len(pl)
    if st == 0 or st == 2:
        r = sh[0] if st == 0 else sh[1]
        seg = np.zeros_like(pl)
        if st == 2:
            ax = 0 if "capsule_x" in variant else 1
            seg[:, ax] = np.clip(pl[:, ax], -sh[0], sh[0])
        dl = pl - seg
        n = np.linalg.norm(dl, axis=1)
        zero = n == 0.0
        nn = np.where(zero, 1.0, n)
        proj = seg + dl * (r / nn)[:, None]
        # at the centre / on the segment every direction is closest: the library picks +y (ball), +x (capsule)
        proj[zero, 1 if st == 0 else 0] += r
        return proj, n - r, np.where(zero, 1.0, np.maximum(1.0, r / nn))
    he = sh[:d]
    q = np.abs(pl) - he
    outside = np.any(q > 0.0, axis=1)
    proj = np.clip(pl, -he, he)
    sd = np.where(outside, np.linalg.norm(np.maximum(q, 0.0), axis=1), q.max(1))
    k = np.argmin(q, axis=1) if "cuboid_farthest_face" in variant else np.argmax(q, axis=1)   # face of least penetration
    ins = ~outside
    face = np.where(pl[ins, k[ins]] > 0.0, 1.0, -1.0) * he[k[ins]]
    pin = pl[ins].copy()
    pin[np.arange(len(pin)), k[ins]] = face
    proj[ins] = pin
    return proj, sd, np.ones(M)


class NodeField:
    """Truth of the node cdf at world cells [M, d] for colliders (list of colliders_of records).

    aff, dist, closest: what the kernel stores. b_dist [M]: bound of `dist`. und_bits [M]: the affinity / sign bits an
    fp32 evaluation may decide either way; und_dist [M]: the voter set is undecided (distance and closest id are then
    not compared); und_tie [M]: two voters tie for the closest id within their bounds.

    rigid: the mesh_truth.Rigid of the scene's mesh colliders at the same poses (None: mesh colliders leave no trace, as
    without one); it fills their columns, which merge like the analytic ones."""

    def __init__(self, cols, d, h, cells, u=U32, variant=(), rigid=None):
        cells = np.asarray(cells, np.int64)
        M = len(cells)
        self.d, self.h, self.cells = d, float(h), cells
        self.keys = T.node_key(cells)
        assert np.all(np.diff(self.keys) > 0) or M < 2, "cells must be sorted lexicographically and unique"
        pt = cells * self.h
        cap = 1.5 * self.h
        nc = min(len(cols), MAXC)
        big = np.full((M, max(nc, 1)), np.inf)
        dist_c, b_c = big.copy(), np.zeros_like(big)
        voter = np.zeros_like(big, bool)
        inside = voter.copy()
        aff_und, in_und, exact_c, dist_und = voter.copy(), voter.copy(), voter.copy(), voter.copy()
        self.sd = big.copy()
        for i in range(nc):
            c = cols[i]
            if c["shape_type"] >= 3:
                continue
            s = 1.0 if "ignore_scale" in variant else c["scale"]
            R, t = c["R"], c["trans"]
            pl = ((pt - t) @ R) / s
            projl, sd, amp = _project(c, pl, d, variant)
            Rw = R.T if "inverse_rot_to_world" in variant else R
            dv = (projl * s) @ Rw.T + t - pt
            a = np.abs(dv)
            dist = np.linalg.norm(dv, axis=1)
            ins = sd <= 0.0
            within = dist <= cap if "euclid_within" in variant else np.all(a <= cap, axis=1)
            extent = {0: c["shape"][0], 1: np.linalg.norm(c["shape"][:d]), 2: c["shape"][0] + c["shape"][1]}[c["shape_type"]]
            near = np.linalg.norm(pt - t, axis=1) + s * extent
            far = np.linalg.norm(pt, axis=1) + np.linalg.norm(t)
            exact = _is_exact(c, d, self.h)
            b = np.zeros(M) if exact else u * ((C_FAR if not T._pow2(self.h) else C_FAR - 2.0) * far + C_NEAR[d] * near)
            bv = b * amp                                   # bound of every component of proj - pt
            e = bv + np.where(bv > 0, 2.0 * u * cap, 0.0)  # ... against cap = fl(1.5 fl(h))
            iu = (np.abs(sd * s) <= bv) & (bv > 0)
            w_true = np.all((a < cap - e[:, None]) | ((e[:, None] == 0) & (a <= cap)), axis=1)
            w_false = np.any(a > cap + e[:, None], axis=1)
            if "euclid_within" in variant:
                w_true, w_false = within, ~within
            au = ~((ins & ~iu) | w_true) & ~((~ins & ~iu) & w_false)
            # the distance: an error along the normal counts in full, one tangent to the boundary to second order
            bt = bv - b
            with np.errstate(divide="ignore", invalid="ignore"):
                b_d = b + np.minimum(bt, np.where(dist > 0, bt * bt / dist, bt)) + C_DIST * u * dist
            voter[:, i], inside[:, i], dist_c[:, i], b_c[:, i] = ins | within, ins, dist, b_d
            aff_und[:, i], in_und[:, i], exact_c[:, i] = au, iu, exact
            self.sd[:, i] = sd * s
        if rigid is not None:
            rigid.fill(cells, nc, voter, inside, dist_c, b_c, aff_und, in_und, exact_c, dist_und)
        dm = np.where(voter, dist_c, np.inf)
        dmin = dm.min(1)
        any_v = np.isfinite(dmin)
        first = np.argmin(dm, axis=1)
        if "closest_highest" in variant:
            first = dm.shape[1] - 1 - np.argmin(dm[:, ::-1], axis=1)
        self.dist = np.where(any_v, dmin, NO_VOTER)
        self.closest = np.where(any_v, first, NONE).astype(np.uint32)
        sh = np.arange(dm.shape[1], dtype=np.uint32)
        self.aff = ((voter.astype(np.uint32) << sh) | (inside.astype(np.uint32) << (sh + 16))).sum(1).astype(np.uint32) if nc else np.zeros(M, np.uint32)
        self.und_bits = ((aff_und.astype(np.uint32) << sh) | (in_und.astype(np.uint32) << (sh + 16))).sum(1).astype(np.uint32) if nc else np.zeros(M, np.uint32)
        self.und_dist = aff_und.any(1) | dist_und.any(1)
        # ties for the closest id: another voter within the two bounds of the minimum (equal and exact: decided, lowest id)
        rows = np.arange(M)
        bmin = b_c[rows, first]
        close = voter & (dm <= (dmin + bmin)[:, None] + b_c) & any_v[:, None]
        close[rows, first] = False
        decided_tie = close & (dm == dmin[:, None]) & exact_c & exact_c[rows, first][:, None]
        self.und_tie = (close & ~decided_tie).any(1)
        self.b_dist = np.where(any_v, np.max(np.where(close | (np.arange(dm.shape[1])[None, :] == first[:, None]), b_c, 0.0), axis=1), 0.0)
        self.voter, self.inside, self.dist_c = voter, inside, dist_c

    @property
    def undecided(self):
        return (self.und_bits != 0) | self.und_tie

    @property
    def carries(self):
        """nodes that carry any affinity (or may)"""
        return (self.aff != 0) | (self.und_bits != 0)

    def share(self):
        return int(self.undecided.sum()), int(self.carries.sum())


def check_nodes(tag, nf: NodeField, dist, aff, closest, fails):
    """Every node of a field (arrays in the order of nf.cells) against the truth: bits exact outside the undecided set,
    distance within its bound, nodes with no voter exactly (1e10, NONE, 0)."""
    dist = np.asarray(dist, np.float64)
    aff = np.asarray(aff, np.uint32)
    closest = np.asarray(closest, np.uint32)
    assert len(dist) == len(nf.cells)
    if not np.all(np.isfinite(dist)):
        fails.append(f"{tag}: non-finite node distance")
    wrong = (aff ^ nf.aff) & ~nf.und_bits
    if wrong.any():
        i = int(np.argmax(wrong != 0))
        fails.append(f"{tag}: {int((wrong != 0).sum())} nodes with wrong decided affinity / sign bits "
                     f"(first cell {nf.cells[i].tolist()}: {int(aff[i]):#x} vs {int(nf.aff[i]):#x}, undecided {int(nf.und_bits[i]):#x})")
    sure = ~nf.und_dist
    none = sure & (nf.aff == 0)
    bad = none & ((dist != NO_VOTER) | (closest != NONE) | (aff != 0))
    if bad.any():
        fails.append(f"{tag}: {int(bad.sum())} nodes with no voter do not hold (1e10, NONE, 0)")
    idc = sure & ~nf.und_tie
    if (closest[idc] != nf.closest[idc]).any():
        i = int(np.nonzero(idc)[0][np.argmax(closest[idc] != nf.closest[idc])])
        fails.append(f"{tag}: {int((closest[idc] != nf.closest[idc]).sum())} wrong closest ids (first cell {nf.cells[i].tolist()}: "
                     f"{int(closest[i])} vs {int(nf.closest[i])})")
    sel = sure & (nf.aff != 0)
    T.check(f"{tag}: node distance (scale |pt| + |trans| + scale extent)", np.abs(dist - nf.dist), nf.b_dist, fails, sel)
    return nf.share()


# ------------------------------------------------------------------------------------------------ particle field
class _Pos:
    def __init__(self, pos):
        self.pos32 = np.ascontiguousarray(pos, np.float32)
        self.n, self.d = self.pos32.shape
        self.x = self.pos32.astype(np.float64)


def _det(m):
    return np.linalg.det(m)


class ParticleField:
    """g2p_cdf.wgsl:39-250 in fp64 from a node field given as arrays over sorted world cells: `ndist`, `naff` (stencil nodes
    that are not among the cells read as affinity 0). `prev_aff`: the particles' previous affinity words (sign persistence).
    `node_b`, `node_und`: the bound of the node distances and the nodes' undecided bits (end-to-end use; None for a field
    taken as exact: the isolated use).

    aff, dist, normal: what the kernel stores. b_dist, b_normal: their bounds. undecided: either outcome accepted."""

    def __init__(self, pos, h, cells, ndist, naff, prev_aff=None, node_b=None, node_und=None, u=U32, variant=()):
        P = _Pos(pos)
        n, d = P.n, P.d
        h = float(h)
        st = T.Stencil(P, h)
        self.st, self.d, self.h, self.n = st, d, h, n
        keys = T.node_key(np.asarray(cells, np.int64))
        want = T.node_key(st.node.reshape(-1, d))
        j = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
        hit = (keys[j] == want) if len(keys) else np.zeros(len(want), bool)
        S = st.w.shape[1]
        na = np.where(hit, np.asarray(naff, np.uint32)[j], 0).astype(np.uint32).reshape(n, S)
        nd = np.where(hit, np.asarray(ndist, np.float64)[j], 0.0).reshape(n, S)
        nb = np.zeros((n, S)) if node_b is None else np.where(hit, np.asarray(node_b, np.float64)[j], 0.0).reshape(n, S)
        nu = np.zeros((n, S), np.uint32) if node_und is None else np.where(hit, np.asarray(node_und, np.uint32)[j], 0).astype(np.uint32).reshape(n, S)
        prev = np.zeros(n, np.uint32) if prev_aff is None or "no_persistence" in variant else np.asarray(prev_aff, np.uint32)
        w = st.w
        # absolute error of a kernel's weights: per axis dt = u (2 |cell| [cell * h and the fp32 h, unless h is a power of two]
        # + C_ABS_T), dw <= |w'(t)| dt + dt^2 (|w''| <= 2); the product of D factors, and the D - 1 roundings of the product
        cell = st.node[:, 0, :]
        dt = u * ((0.0 if T._pow2(h) else 2.0) * np.abs(cell) + C_ABS_T)                 # [n, d]
        w1 = eval_all(-st.ref / h)                                                       # [n, d, 3]
        shf = T.shifts_of(d)
        dw = np.zeros((n, S))
        tt = -st.ref / h
        dw1 = np.abs(np.stack([tt - 1.5, -2.0 * (tt - 1.0), tt - 0.5], axis=-1)) * dt[:, :, None] + (dt * dt)[:, :, None]   # |w'| dt + dt^2
        for k in range(d):
            f = dw1[:, k, shf[:, k]]
            for q in range(d):
                if q != k:
                    f = f * w1[:, q, shf[:, q]]
            dw += f
        dw += d * u * w
        dwp = dw + w * dt.sum(1)[:, None]               # ... and of pv = ref + shift h relative to h, carried as a weight error
        # ---- pass 1: union of affinities, sign votes
        paff = np.bitwise_or.reduce(na & np.uint32(0xffff), axis=1)
        und = (nu != 0).any(1)
        self.why = dict(node=und.copy())
        und_vote = np.zeros(n, bool)
        self.vote = np.zeros((n, MAXC))
        self.b_vote = np.zeros((n, MAXC))
        signs = np.zeros(n, np.uint32)
        absd = np.abs(nd)
        for c in range(MAXC):
            has = ((na >> np.uint32(c)) & 1).astype(bool)
            if not has.any() and not ((prev >> np.uint32(c)) & 1).any():
                continue
            sg = np.where(((na >> np.uint32(16 + c)) & 1).astype(bool), -1.0, 1.0)
            vote = np.where(has, w * sg * nd, 0.0).sum(1)
            bvote = C_VOTE[d] * u * np.where(has, w * absd, 0.0).sum(1) + np.where(has, dw * absd + w * nb, 0.0).sum(1)
            fresh = ((prev >> np.uint32(c)) & 1) == 0
            bit = np.where(fresh, vote < 0.0, ((prev >> np.uint32(16 + c)) & 1).astype(bool))
            signs |= bit.astype(np.uint32) << np.uint32(16 + c)
            # (a vote of exact zeros, every term w * 0 with nothing to round, is decided: not negative)
            und_vote |= fresh & has.any(1) & (np.abs(vote) <= bvote) & ~((bvote == 0.0) & (vote == 0.0))
            self.vote[:, c], self.b_vote[:, c] = vote, bvote
        und |= und_vote
        self.why['vote'] = und_vote
        full = paff | signs
        # ---- pass 2: weighted least squares for (grad d, d)
        comb = na & full[:, None] & np.uint32(0xffff)
        use = comb != 0
        sdiff = ((na >> np.uint32(16)) ^ (full[:, None] >> np.uint32(16))) & comb
        dd = np.where(sdiff == 0, nd, -nd)
        pv = np.concatenate([st.dpt, np.ones((n, S, 1))], axis=2)                    # [n, S, d + 1]
        wu = np.where(use, w, 0.0)
        G = np.einsum("ns,nsr,nsc->nrc", wu, pv, pv)
        rhs = np.einsum("ns,nsr,ns->nr", wu, pv, dd)
        if "unmirrored" in variant:
            G[:, 0, 1] = 0.0
        det = _det(G)
        N = d + 1
        diag = np.einsum("nii->ni", G)
        qe = np.einsum("ns,nsr->nr", np.where(use, dwp, 0.0), pv * pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho2 = np.where(diag > 0, qe / diag, 0.0).max(1)
        self.b_det = math.factorial(N) * N * (rho2 + (3 ** d + 6) * u) * np.prod(diag, axis=1)
        self.why['det'] = np.abs(det - 1.0e-8) <= self.b_det
        und |= self.why['det']
        ok = det > 1.0e-8
        self.det = det
        sol = np.zeros((n, N))
        kappa = np.ones(n)
        bx = np.zeros((n, N))                            # componentwise bound of the solution, scaled unknowns (h grad, d)
        sc = np.array([h] * d + [1.0])
        if ok.any():
            Gs = G[ok] / sc[None, :, None] / sc[None, None, :]
            Gi = np.linalg.inv(Gs)
            xs = np.einsum("nrc,nc->nr", Gi, rhs[ok] / sc[None, :])
            sol[ok] = xs / sc[None, :]
            ev = np.linalg.eigvalsh(0.5 * (Gs + Gs.transpose(0, 2, 1)))
            kappa[ok] = ev[:, -1] / np.maximum(ev[:, 0], 1e-300)
            # |dx| <= |G^-1| (|dr| + |dG| |x|), entry by entry (Bauer / Skeel): an entry of G or of the right-hand side is a sum
            # of 3^D products accumulated in fp32 (C_ACC u of its terms' magnitudes) of weights that carry their own
            # error (dwp) and of node distances that carry theirs (nb); the LDL^T solve is backward stable entry by entry,
            # |dG| <= C_SOLVE u |G| (its (D + 1)^2 multiply-subtracts twice over: factorisation and substitutions)
            A = np.abs(pv[ok]) / sc[None, None, :]
            wa = np.where(use[ok], C_ACC[d] * u * w[ok] + dwp[ok], 0.0)
            ax = np.abs(xs)
            dr = np.einsum("ns,nsr,ns->nr", wa, A, absd[ok]) + np.einsum("ns,nsr,ns->nr", wu[ok], A, nb[ok])
            dG = np.einsum("ns,nsr,nsc->nrc", wa, A, A) + C_SOLVE[d] * u * np.abs(Gs)
            bx[ok] = np.einsum("nrc,nc->nr", np.abs(Gi), dr + np.einsum("nrc,nc->nr", dG, ax))
        self.cond = kappa
        grad = sol[:, :d]
        ln = np.linalg.norm(grad, axis=1)
        self.b_dist = np.where(ok, bx[:, d], 0.0)
        b_grad = np.linalg.norm(bx[:, :d], axis=1) / h
        with np.errstate(divide="ignore", invalid="ignore"):
            normal = np.where(ok[:, None] & (ln > 0)[:, None], grad / ln[:, None], 0.0)
            self.b_normal = np.where(ok, np.where(ln > 0, 2.0 * b_grad / ln, np.inf) + 4.0 * u, 0.0)
        if d == 2:
            tiny = ok & ~(ln > 1.0e-6)
            normal[tiny] = 0.0
            und |= ok & (np.abs(ln - 1.0e-6) <= b_grad)
        self.aff = np.where(ok, full, 0).astype(np.uint32)
        self.dist = np.where(ok, sol[:, d], 0.0)
        self.normal = normal
        self.grad_len = ln
        if "swap_dist_normal0" in variant:
            self.dist, self.normal = self.normal[:, 0].copy(), np.concatenate([self.dist[:, None], self.normal[:, 1:]], axis=1)
        self.ok, self.paff, self.undecided = ok, paff, und
        self.reaches = paff != 0                         # particles with a collider-affine node in their stencil
        self.fresh_sign_differs = None
        if prev_aff is not None:
            fresh_bits = np.zeros(n, np.uint32)
            for c in range(MAXC):
                fresh_bits |= ((self.vote[:, c] < 0.0).astype(np.uint32) << np.uint32(16 + c))
            m = (paff.astype(np.uint32) << np.uint32(16))
            self.fresh_sign_differs = ok & (((fresh_bits ^ self.aff) & m) != 0) & ~und

    def share(self):
        return int((self.undecided & self.reaches).sum()), int(self.reaches.sum())


def check_particle_cdf(tag, pf: ParticleField, aff, dist, normal, fails, sel=None):
    """cdf_affinity exact for decided particles, cdf_dist and cdf_normal within their bounds"""
    aff = np.asarray(aff, np.uint32)
    dist = np.asarray(dist, np.float64)
    normal = np.asarray(normal, np.float64)
    if not (np.all(np.isfinite(dist)) and np.all(np.isfinite(normal))):
        fails.append(f"{tag}: non-finite particle cdf")
    dec = ~pf.undecided if sel is None else (~pf.undecided & sel)
    bad = dec & (aff != pf.aff)
    if bad.any():
        i = int(np.argmax(bad))
        fails.append(f"{tag}: {int(bad.sum())} decided particles with a wrong affinity word (first #{i}: {int(aff[i]):#x} vs {int(pf.aff[i]):#x}, "
                     f"det {pf.det[i]:.3e})")
    T.check(f"{tag}: cdf_dist (scale |G^-1| (sum w |d| + |G| |x|))", np.abs(dist - pf.dist), pf.b_dist, fails, dec)
    T.check(f"{tag}: cdf_normal (the same / (h |grad|))", np.linalg.norm(normal - pf.normal, axis=1), pf.b_normal, fails, dec)
    return pf.share()


def from_truth_nodes(pos, h, nf: NodeField, prev_aff=None, variant=()):
    """the end-to-end particle truth: from the truth's node field, its bounds and undecided bits propagated"""
    # A node whose sign bit alone is undecided lies within its bound of the boundary: either sign moves a vote or a
    # right-hand side by 2 w |d| <= 2 w b at most, which the node bound carries; an undecided affinity bit changes what
    # the particle fits, and leaves the particle undecided.
    sign_und = (nf.und_bits >> np.uint32(16)) != 0
    nb = np.where(nf.aff != 0, nf.b_dist, 0.0) + np.where(sign_und, 2.0 * np.abs(np.where(nf.dist < NO_VOTER, nf.dist, 0.0)), 0.0)
    return ParticleField(pos, h, nf.cells, nf.dist, nf.aff, prev_aff, node_b=nb, node_und=nf.und_bits & np.uint32(0xffff), variant=variant)


def active_cells(pos32, h, d, rigid=None):
    """world cells of the nodes of the active blocks (the associated block of every particle and its + neighbours; with
    `rigid`, a mesh_truth.Rigid, the blocks its samples add to them as well), sorted"""
    if rigid is not None:
        return block_cells(rigid.set_particles(pos32), d)
    bw = T.bw_of(d)
    blk = assoc_cell(np.asarray(pos32, np.float32), h) // bw
    offs = np.unique(T.shifts_of(d) % 2, axis=0)
    blocks = np.unique((blk[:, None, :] + offs[None, :, :]).reshape(-1, d), axis=0)
    return block_cells(blocks, d)


# ------------------------------------------------------------------------------------------------ scenes
NODE_CAP = 0.02       # undecided share of the nodes that carry any affinity
PART_CAP = 0.05       # undecided share of the particles that reach a collider-affine node (a subset of the particles in
                      # near-collider blocks: the smaller denominator makes the cap stricter)
DET_EDGE_CAP = 0.25


def _quat(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(deg) / 2.0
    return tuple(float(v) for v in f32(np.append(a * math.sin(t), math.cos(t))))


def ident(d):
    """the identity rotation as a Collider takes it: the angle 0 / the quaternion (0, 0, 0, 1)"""
    return (0.0,) if d == 2 else (0.0, 0.0, 0.0, 1.0)


def _rot(d, deg=33.0):
    return (float(np.float32(math.radians(deg))),) if d == 2 else _quat((1.0, 2.0, 3.0), deg)


def _v(x, d):
    return tuple(float(v) for v in f32(np.asarray(x, np.float64)[:d]))


RIM = 1.0             # distance (in h) up to which a particle's stencil holds two layers of collider-affine nodes at least
RIM_KEEP = 0.02
RIM_H = 0.25


def signed_distance(cols, x, d):
    """world signed distance of points x [n, d] to the nearest of the first 16 analytic colliders"""
    out = np.full(len(x), np.inf)
    for c in cols[:MAXC]:
        if c["shape_type"] < 3:
            out = np.minimum(out, _project(c, ((x - c["trans"]) @ c["R"]) / c["scale"], d, ())[1] * c["scale"])
    return out


def _static(d, h, rng, colliders, boxes, n, uniform=False, keep=None, rim_keep=None, rim_units=None):
    """n particles at rest (v = 0, C = 0, F = I, no gravity) uniformly in the union of the boxes [(lo, hi)].
    A particle at the rim of a collider's reach has one layer of collider-affine nodes in its stencil: its Gram matrix
    is singular, and whether an fp32 determinant of it passes the absolute 1e-8 test depends on h (at h = 2 it is noise
    of 1e-7). Such particles are undecided by nature; of the candidates farther than RIM h from every collider the
    scenes keep `rim_keep`, so n counts candidates, not particles. Where h makes them decidable (h <= RIM_H: the noise
    of the determinant, ~3000 u (h^2 / 4)^D, stays below 1e-8) all are kept by default.
    `rim_units`: the distance of fp32 positions to the colliders in units of the rim (scenes with mesh colliders, whose
    reach is their samples' stencil: mesh_truth.rim_units); default: the analytic signed distance / (RIM h)."""
    if rim_keep is None:
        rim_keep = 1.0 if h <= RIM_H else RIM_KEEP
    from wgsparkl_amd.solver import SimulationParams
    vol = np.array([np.prod(np.asarray(hi[:d], np.float64) - np.asarray(lo[:d], np.float64)) for lo, hi in boxes])
    cnt = np.maximum(1, np.rint(n * vol / vol.sum())).astype(int)
    pos = np.concatenate([rng.uniform(np.asarray(lo[:d], np.float64), np.asarray(hi[:d], np.float64), (k, d)) for (lo, hi), k in zip(boxes, cnt)])
    if keep is not None:
        pos = pos[keep(pos)]
    x32 = pos.astype(np.float32).astype(np.float64)
    sd = signed_distance(colliders_of(colliders, d), x32, d) / h if rim_units is None else rim_units(x32) * RIM
    pos = pos[(sd <= RIM) | (rng.random(len(pos)) < rim_keep)]
    sc = T._finish(pos, h, rng, vel=np.zeros_like(pos), uniform=uniform, vel_scale=0.0)
    ps = sc["particles"]
    ps.affine[:] = 0.0
    ps.def_grad[:] = np.eye(d, dtype=np.float32).reshape(-1)
    sc["params"] = SimulationParams(gravity=(0.0,) * d, dt=T.DT)
    sc["colliders"] = list(colliders)
    sc["grid_capacity"] = max(sc["grid_capacity"], 256)
    return sc


def _n(d):
    return 12000 if d == 3 else 3000


def ball(d, h, seed=0, **kw):
    """a ball of radius 2.3 h at a non-dyadic centre, one of radius 0.4 h (smaller than a cell), and one centred exactly on
    the node at the origin (the n == 0 branch), which no particle reaches"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    c0 = np.array([5.37, 5.21, 5.13]) * h
    c1 = c0 + np.array([4.1, 0.3, -0.2]) * h
    cols = [Collider.ball(float(np.float32(2.3 * h)), _v(c0, d)), Collider.ball(float(np.float32(0.4 * h)), _v(c1, d)),
            Collider.ball(float(np.float32(0.3 * h)), (0.0,) * d)]
    keep = lambda p: ~np.all(p < 2.6 * h, axis=1)
    return _static(d, h, rng, cols, [(c0 - 4.6 * h, c1 + np.array([2.5, 4.3, 4.8]) * h)], _n(d), keep=keep, **kw)


def capsule(d, h, seed=1, **kw):
    """a capsule (half height 1.5 h, radius 0.8 h) scaled by 1.7, rotated by 33 degrees (3D: about (1, 2, 3))"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    c0 = np.array([7.37, 7.21, 7.13]) * h
    cols = [Collider(2, (float(np.float32(1.5 * h)), float(np.float32(0.8 * h))), _v(c0, d), rotation=_rot(d), scale=float(np.float32(1.7)))]
    return _static(d, h, rng, cols, [(c0 - 6.0 * h, c0 + 6.0 * h)], _n(d), **kw)


def cuboid(d, h, seed=2, offset_blocks=None, he=(2.3, 0.7, 1.4), frac=(5.37, 5.21, 5.13), **kw):
    """a rotated cuboid of unequal half extents (2.3, 0.7, 1.4) h, one below h; particles inside and outside"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    c0 = np.array(frac) * h
    if offset_blocks is not None:
        c0[:d] += np.asarray(offset_blocks, np.float64)[:d] * T.bw_of(d) * h
    cols = [Collider.cuboid(_v(np.array(he) * h, d), _v(c0, d), rotation=_rot(d))]
    r = np.linalg.norm(np.array(he)[:d]) + 2.2
    return _static(d, h, rng, cols, [(c0 - r * h, c0 + r * h)], _n(d), **kw)


def aligned(d, h, seed=3, **kw):
    """an axis-aligned cuboid at translation 0 whose faces lie on node planes: inside by equality (exact when h is a power
    of two)"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    rot = ident(d)
    he = np.array([2.0, 1.0, 2.0]) if T._pow2(h) else np.array([2.25, 1.25, 2.25])    # (other h: no node can lie on a face exactly)
    cols = [Collider.cuboid(_v(he * h, d), (0.0,) * d, rotation=rot)]
    return _static(d, h, rng, cols, [(np.full(3, -4.4 * h), np.full(3, 4.4 * h))], _n(d), **kw)


def two_equal(d, h, seed=4, **kw):
    """two axis-aligned cuboids whose facing faces lie 0.75 h either side of the node plane x = 4 h, overlapping in y over
    the node row y = 0 only: those nodes tie for the closest id (exactly when h is a power of two); a ball next to them puts
    nodes in reach of three colliders"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    rot = ident(d)
    he = _v(np.array([1.5, 2.0, 1.25]) * h, d)
    cols = [Collider.cuboid(he, _v(np.array([1.75, -1.75, 0.0]) * h, d), rotation=rot),
            Collider.cuboid(he, _v(np.array([6.25, 1.75, 0.0]) * h, d), rotation=rot),
            Collider.ball(float(np.float32(0.9 * h)), _v(np.array([4.13, 2.1, 0.2]) * h, d))]
    return _static(d, h, rng, cols, [(np.array([-2.4, -6.2, -3.4]) * h, np.array([10.4, 6.2, 3.4]) * h)], _n(d), **kw)


def sixteen(d, h, seed=5, **kw):
    """17 small balls in a row: the 17th (index 16) leaves no trace"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    cols = [Collider.ball(float(np.float32(0.45 * h)), _v(np.array([1.31 + 2.5 * i, 2.23, 2.17]) * h, d)) for i in range(17)]
    return _static(d, h, rng, cols, [(np.array([-1.4, -0.4, -0.4]) * h, np.array([43.9, 4.9, 4.9]) * h)], _n(d), **kw)


FAR_BLOCKS = {3: (1000, -500, -1000), 2: (1000, -1000)}
FAR_BLOCKS_NOT_POW2 = {3: (100, -50, -100), 2: (100, -100)}


def far_blocks(d, h):
    return (FAR_BLOCKS if T._pow2(h) else FAR_BLOCKS_NOT_POW2)[d]


def far(d, h, seed=6, **kw):
    """the cuboid scene at block coordinates (1000, -500, -1000) (3D) / (1000, -1000) (2D).
    2D: at 30000 blocks one fp32 spacing of a coordinate is 0.03 h, and the share of nodes within the bound of a
    threshold cannot meet NODE_CAP whatever the pose; the cap is a condition on the scenes, so the scene moved in.
    When h is no power of two, cell * h is rounded and a kernel's weights are off by 2 |cell| u: at 4000 cells the
    determinant of a partial stencil is uncertain by more than the 1e-8 it is tested against at h = 0.2, and PART_CAP
    cannot hold; those cases sit at a tenth of the distance."""
    kw.setdefault("rim_keep", RIM_KEEP)              # (far from the origin the weights' own error makes the rim undecided at every h)
    return cuboid(d, h, seed=seed, offset_blocks=far_blocks(d, h), frac=(5.41, 5.17, 5.13), **kw)


def far_nodes(d, h=0.2, seed=6):
    """the far scene at the full distance whatever h: what the node checks run on where `far` itself had to move in"""
    # (a larger cuboid than the scene's: in 2D that one has 40 collider-affine nodes, and one undecided node is 2.5 % of them)
    return cuboid(d, h, seed=seed, offset_blocks=FAR_BLOCKS[d], frac=(5.41, 5.17, 5.13), he=(9.3, 4.7, 1.4), rim_keep=RIM_KEEP)


def det_edge(h=0.1, seed=7, **kw):
    """3D, h = 0.1: det of the full-stencil Gram matrix is ~(h^2 / 4)^3 = 1.6e-8, so particles at the rim of a collider's
    reach (partial stencils) fall below 1e-8 and take the default cdf"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    c0 = np.array([5.37, 5.21, 5.13]) * h
    cols = [Collider.cuboid(_v(np.array([2.3, 1.7, 1.4]) * h, 3), _v(c0, 3), rotation=_rot(3))]
    return _static(3, h, rng, cols, [(c0 - 5.5 * h, c0 + 5.5 * h)], 4000, rim_keep=1.0, **kw)


SCENES = dict(ball=ball, capsule=capsule, cuboid=cuboid, aligned=aligned, two_equal=two_equal, sixteen=sixteen, far=far)
HS = (0.2, 0.5, 2.0)


class Truth(NamedTuple):
    """what truth_of returns"""
    rigid: Optional[object]        # the mesh_truth.Rigid of the scene's mesh colliders (None without one)
    nodes: NodeField
    particles: ParticleField       # end to end: from `nodes`


def truth_of(sc, cells=None, poses=None, prev_aff=None, pos=None, colliders=None, variant=()):
    """the Truth of a scene at its uploaded (or given) positions, poses and colliders; the nodes are those of the active
    cells (with mesh colliders: the blocks their samples add included) unless `cells` are given"""
    from mesh_truth import rigid_of
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    pos = ps.pos if pos is None else pos
    rg = rigid_of(sc, poses, colliders, variant)
    cols = colliders_of(colliders or sc["colliders"], d, poses)
    nf = NodeField(cols, d, h, active_cells(pos, h, d, rigid=rg) if cells is None else cells, rigid=rg, variant=variant)
    return Truth(rg, nf, from_truth_nodes(pos, h, nf, prev_aff, variant=variant))


def assert_caps(tag, nf: NodeField, pf: ParticleField, part_cap=PART_CAP):
    un, cn = nf.share()
    up, cp = pf.share()
    report_margin(f"{tag}: undecided share of the nodes that carry an affinity", un / max(cn, 1), NODE_CAP, count=un, of=cn)
    report_margin(f"{tag}: undecided share of the particles that reach a collider", up / max(cp, 1), part_cap, count=up, of=cp)
    assert cn > 0 and cp > 0, f"{tag}: no node / particle near a collider"
    assert un <= NODE_CAP * cn, f"{tag}: {un} of {cn} affinity-carrying nodes are undecided"
    assert up <= part_cap * cp, f"{tag}: {up} of {cp} near-collider particles are undecided"


# ------------------------------------------------------------------------------------------------ the C oracle beside the truth
REL = 1.0e-10
_CACHE = {}


def _prev(sc, seed=11):
    """previous affinity words: a third of the particles carried collider 0 with a positive sign, a third with a negative one"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0x1, 0x10001], np.uint32), sc["particles"].n)


class Case(NamedTuple):
    sc: dict
    prev: np.ndarray               # the particles' previous affinity words (_prev)
    truth: Truth


def _case(make, d, h):
    """the Case of the scene builder `make` (an entry of a SCENES table), built once per process"""
    key = (make, d, h)
    if key not in _CACHE:
        sc = make(d, h)
        prev = _prev(sc)
        _CACHE[key] = Case(sc, prev, truth_of(sc, prev_aff=prev))
    return _CACHE[key]


def _oracle_fields(sc, dtype, prev):
    """The distance fields of the C oracle, run pass by pass in the order of orc_step_full: update_rigid_particles,
    sort_rigid, grid_update_cdf, p2g_cdf, g2p_cdf. Without a mesh collider update_rigid_particles and p2g_cdf do nothing and
    sort_rigid is sort (oracle/orc.py), which leaves the analytic sequence sort, grid_update_cdf, g2p_cdf."""
    ps = sc["particles"]
    st = oracle(ps.dim, dtype).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], 0)
    st.arr["cdf_affinity"][:] = prev
    st.update_rigid_particles()
    st.sort_rigid()
    assert not st.overflow
    st.grid_update_cdf()
    st.p2g_cdf()
    st.g2p_cdf()
    cells, _, dist, aff, closest = st.grid_records()
    return dict(cells=cells, dist=dist, aff=aff, closest=closest, paff=st.arr["cdf_affinity"].copy(),
                pdist=st.arr["cdf_dist"].copy(), pnormal=st.arr["cdf_normal"].copy())


def assert_matches_fp64_oracle(sc, prev, truth: Truth):
    """the truth's active cells, node field and particle field are the C fp64 oracle's: bits equal outside the undecided sets,
    distances and normals to REL"""
    nf, pf = truth.nodes, truth.particles
    h = sc["cell_width"]
    o = _oracle_fields(sc, np.float64, prev)
    assert np.array_equal(o["cells"], nf.cells), "the truth's active cells are not the oracle's"
    assert not ((o["aff"] ^ nf.aff) & ~nf.und_bits).any(), "decided node bits differ"
    sure = ~nf.und_dist
    idc = sure & ~nf.und_tie
    assert np.array_equal(o["closest"][idc], nf.closest[idc])
    assert np.all(np.abs(o["dist"][sure] - nf.dist[sure]) <= REL * np.maximum(np.abs(nf.dist[sure]), h)), \
        float(np.max(np.abs(o["dist"][sure] - nf.dist[sure])))
    # particle field from the oracle's own nodes (isolated) and end to end
    iso = ParticleField(sc["particles"].pos, h, o["cells"], o["dist"], o["aff"], prev)
    for tag, p in (("isolated", iso), ("end to end", pf)):
        dec = ~p.undecided
        assert np.array_equal(o["paff"][dec], p.aff[dec]), f"{tag}: decided particle affinity words differ"
        tol = REL * np.maximum(1.0, p.cond)               # (the fp64 solves themselves differ by cond(G) 2^-53)
        assert np.all(np.abs(o["pdist"] - p.dist)[dec] <= (tol * np.maximum(np.abs(p.dist), h))[dec]), tag
        big = dec & (p.grad_len > 1e-3)
        assert np.all(np.linalg.norm(o["pnormal"] - p.normal, axis=1)[big] <= (tol / np.maximum(p.grad_len, 1e-3))[big]), tag


def assert_fp32_oracle_fits_and_caps_hold(name, sc, prev, truth: Truth):
    """the C fp32 oracle lands inside every bound of the truth, the undecided shares meet the caps and no block's membership
    depends on an undecided sample; `name`: the scene's (the margins of a scene with mesh colliders are named "mesh ...")"""
    rg, nf, pf = truth.rigid, truth.nodes, truth.particles
    d, h = sc["particles"].dim, sc["cell_width"]
    name = f"{'mesh ' if rg is not None else ''}{name} {d}D h={h}"
    tag = f"{name} fp32 oracle"
    assert_caps(f"{name} truth", nf, pf)
    if rg is not None:
        assert not rg.und_blocks, f"blocks whose membership depends on an undecided sample: {rg.und_blocks}"
    o = _oracle_fields(sc, np.float32, prev)
    assert np.array_equal(o["cells"], nf.cells)
    fails = []
    check_nodes(tag, nf, o["dist"], o["aff"], o["closest"], fails)
    iso = ParticleField(sc["particles"].pos, h, o["cells"], o["dist"], o["aff"], prev)
    check_particle_cdf(f"{tag} isolated", iso, o["paff"], o["pdist"], o["pnormal"], fails)
    check_particle_cdf(f"{tag} end to end", pf, o["paff"], o["pdist"], o["pnormal"], fails)
    assert not fails, "\n".join(fails)
