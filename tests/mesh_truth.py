"""fp64 truth of the node distance field of mesh colliders (trimesh, heightfield, polyline): which blocks the surface
samples add, which (sample, node) pairs vote, what a vote says, and how the votes of a collider combine at a node. It fills
the per-collider columns that cdf_truth.NodeField merges (the minimum across colliders, the lowest id on ties and the
particle field are that module's, unchanged): cdf_truth.truth_of asks rigid_of here for a scene's Rigid and passes it on.
Shared by tests/test_mesh_truth.py (CPU: the truth against the C fp64 oracle, the bounds against the C fp32 oracle,
perturbations) and tests/test_gpu_mesh_cdf.py (the HIP kernels node by node).

Inputs are what the library receives: the fp32 local samples, primitive vertex ids and fp32 local vertices of
wgsparkl_amd.sampling.build_rigid_particles, the collider records of cdf_truth.colliders_of, h as the Python float.

The rules, from the geometry:
- world points are R (scale local) + trans; a sample's cell is rint(x / h) - 1 per axis;
- a sample adds its own block iff no particle activated it, a particle activated one of its + neighbours, and all of them
  are in key range (not modelled: Rigid.set_particles raises where a sample comes near the range's end); all marks
  against the particle-activated set;
- a sample votes at the 3^D nodes cell + {0, 1, 2}^D, if its own block and the node's block are active;
- 3D: the vote is valid iff the triangle has an area and the three barycentric coordinates of the node's orthogonal
  projection on its plane (2 x 2 Gram system) are >= 0; distance |signed plane distance|, sign bit iff it is < 0, normal
  ab x ac;
- 2D: valid iff the segment has a length and the parameter t of the orthogonal projection on its line is in (0, 1), far
  enough from both ends for the fp32 projection a + ab t to differ from them; Euclidean distance to the projection, sign
  from the left normal (-ab.y, ab.x);
- per collider and node: affinity bit = any valid vote, sign bit = any valid vote with a negative sign, distance = the
  minimum over the valid votes. No `within` cap: the stencil is the cap.

Bounds (fixed multiples of u = 2^-24 times stated scales, settled against the C fp32 oracle in tests/test_mesh_truth.py,
never against the kernels), counted operation by operation:
- a world point: the product by scale (1), the rotation (3D quat_rotate 9, 2D 3), each sum of D components rounded at up
  to sqrt(D) its norm: C_POSE = (1 + 9) sqrt(3) = 18, (1 + 3) sqrt(2) = 6 times |scale local|; the sum with trans: 1 |world|;
- a node: pt = cell * h, the fp32 h and the product: C_PT = 2 |pt| (0 when h is a power of two);
- a sample's x / h: the fp32 h and the division: C_CELL = 2 |x / h| on top of the world point's bound / h;
- a difference of two points is rounded relative to itself: E(p - a) = b(p) + b(a) + u |p - a|;
- n = ab x ac: two products and a difference per component: C_CROSS = 3 sqrt(3) -> 6 |ab| |ac|; a dot product of 3 terms: 3
  products, 2 sums: C_DOT = 5 (2D: 3) times the product of the norms;
- a barycentric numerator (edge e, vector q from one of its ends to the node, |n|^2 times the coordinate):
  dn = Ee (|ab| + |ac|) + C_CROSS u |ab| |ac|;  dt = Ee |n| + |e| dn + C_CROSS u |e| |n|;  dd = dt |q| + |e| |n| E + C_DOT u |e| |n| |q|;
- the signed plane distance n . ap / |n|: (dn (|ap| + |sd|) ) / |n| + E + (C_DOT + 3 [sqrt, division, the norm's own dot]) u |ap|;
- 2D: t = ap . ab / ab . ab: dnum = E |ab| + |ap| Ee + C_DOT2 u |ap| |ab|, dden = 2 |ab| Ee + C_DOT2 u |ab|^2, dt = (dnum + |t| dden) / den
  + u |t|; the projection a + ab t: C_PROJ = 2 (product, sum) times (|a| + |ab|); the distance |p - proj|: an error along the
  normal counts in full, one along the segment to second order, and C_DIST u dist of its own (cdf_truth's).
Contraction into FMAs removes roundings and adds none.
When every operation is exact (mesh_is_exact) the bounds of the decisions are 0: `<=` and `== 0` are decided, not excused."""
from __future__ import annotations

import itertools
import math

import numpy as np

import cdf_truth as CT
import transfer_truth as T
from oracle.np_oracle import assoc_cell, block_cells

U32 = T.U32
C_POSE = {2: 6.0, 3: 18.0}
C_PT = 2.0
C_CELL = 2.0
C_CROSS = 6.0
C_DOT = {2: 3.0, 3: 5.0}
C_PROJ = 2.0
C_DIST = CT.C_DIST


def _f64(a):
    return np.asarray(np.asarray(a, np.float32), np.float64)


def _norm(v):
    return np.linalg.norm(v, axis=-1)


def _granule(vals, h):
    """the coarsest of h, h / 2, ... h / 64 of which every value is a multiple (None: none of them)"""
    for k in range(7):
        q = np.asarray(vals, np.float64) * ((1 << k) / h)
        if np.all(q == np.rint(q)):
            return h / (1 << k)
    return None


def mesh_is_exact(c, local_vtx, d, h):
    """cdf_truth._is_exact for a mesh: every operation of the transform, of the validity tests and of the sign is exact.
    Identity pose, scale 1, h a power of two, vertices and translation on multiples of h / 64 — and few enough of them
    for the integers to stay below 2^24: with g the coarsest granule of h / 2^k the coordinates share, edges of at
    most e g and nodes within 3 h of the surface, the largest intermediate of the barycentric numerators is a sum of
    3 products of (2 e^3) by (e + 3 h / g)."""
    if not T._pow2(h) or c["scale"] != 1.0 or not np.array_equal(c["R"], np.eye(d)):
        return False
    g = _granule(np.concatenate([np.ravel(local_vtx), c["trans"]]), h)
    if g is None:
        return False
    v = np.asarray(local_vtx, np.float64) / g
    e = float(np.max(v.max(0) - v.min(0))) if len(v) else 0.0
    if d == 2:
        return 2.0 * e * (e + 3.0 * h / g) * (e + 3.0 * h / g) < 2 ** 24 and float(np.max(np.abs(v), initial=0.0)) + np.max(np.abs(c["trans"] / g)) < 2 ** 21
    return 6.0 * e ** 3 * (e + 3.0 * h / g) < 2 ** 24 and float(np.max(np.abs(v), initial=0.0)) + np.max(np.abs(c["trans"] / g)) < 2 ** 21


KEY_RANGE = {2: 0x7ffe, 3: 0x1fe}      # |block coordinate| up to which every block is in key range, on the narrowest axis


def _keys(blocks):
    return T.node_key(np.asarray(blocks, np.int64))


class Rigid:
    """The surface samples of a scene's mesh colliders at given poses: world samples and vertices, their bounds, the blocks
    they add to those of the particles (set_particles), and the columns of the node field (fill).

    rb: build_rigid_particles(colliders, d, h); cols: cdf_truth.colliders_of records (the poses before the substep)."""

    def __init__(self, rb, cols, d, h, u=U32, variant=()):
        self.d, self.h, self.u, self.variant = d, float(h), u, tuple(variant)
        ids = np.asarray(rb["ids"], np.int64)
        self.col = ids[:, 3]
        self.prim = ids[:, :d]
        lp, lv = _f64(rb["local_pts"]).reshape(-1, d), _f64(rb["local_vtx"]).reshape(-1, d)
        vcol = np.asarray(rb["vtx_collider"], np.int64)
        self.n = len(lp)
        self.xs, self.vw = np.zeros_like(lp), np.zeros_like(lv)
        self.bx, self.bv = np.zeros(len(lp)), np.zeros(len(lv))
        self.exact = {}          # collider id -> every decision is exact
        for cid in np.unique(vcol):
            c = cols[cid]
            s = 1.0 if "ignore_scale" in variant else c["scale"]
            R, t = c["R"], c["trans"]
            ms, mv = self.col == cid, vcol == cid
            self.xs[ms] = (s * lp[ms]) @ R.T + t
            self.vw[mv] = lv[mv] if "no_pose_vertices" in variant else (s * lv[mv]) @ R.T + t
            ex = mesh_is_exact(c, lv[mv], d, self.h)
            # (identity pose, scale 1, translation 0: the world vertices are the local ones whatever h)
            same = c["scale"] == 1.0 and np.array_equal(R, np.eye(d)) and not np.any(t)
            self.exact[int(cid)] = ex
            self.bv[mv] = 0.0 if (ex or same) else u * (C_POSE[d] * _norm(s * lv[mv]) + _norm(self.vw[mv]))
            self.bx[ms] = 0.0 if same else u * ((0.0 if ex else C_POSE[d]) * _norm(s * lp[ms]) + _norm(self.xs[ms]))
        q = self.xs / self.h
        bq = self.bx[:, None] / self.h + (0.0 if T._pow2(self.h) else C_CELL) * u * np.abs(q)
        self.cell = (np.rint(q) - 1.0).astype(np.int64)
        if "cell_floor" in variant:
            self.cell = (np.floor(q) - 1.0).astype(np.int64)
        self.cell_lo = np.minimum((np.rint(q - bq) - 1.0).astype(np.int64), self.cell)
        self.cell_hi = np.maximum((np.rint(q + bq) - 1.0).astype(np.int64), self.cell)
        self.und_cell = np.any(self.cell_lo != self.cell_hi, axis=1)
        self.blocks = None

    # ------------------------------------------------------------------------------------------ blocks
    def _adds(self, own, pkeys):
        d = self.d
        offs = np.unique(T.shifts_of(d) % 2, axis=0)
        offs = offs[np.any(offs != 0, axis=1)]
        has = np.isin(_keys(own), pkeys)
        nb = np.zeros(len(own), bool)
        for o in offs:
            nb |= np.isin(_keys(own + o[None, :]), pkeys)
        return ~has & nb

    def set_particles(self, pos32):
        """the particle-activated blocks, the blocks the samples add, and what depends on an undecided sample"""
        d, bw = self.d, T.bw_of(self.d)
        blk = assoc_cell(np.asarray(pos32, np.float32), self.h) // bw
        offs = np.unique(T.shifts_of(d) % 2, axis=0)
        pb = np.unique((blk[:, None, :] + offs[None, :, :]).reshape(-1, d), axis=0)
        pkeys = _keys(pb)
        own = self.cell // bw
        # the block rule also asks for the sample's block and its + neighbours to be in key range; that is not modelled
        if len(own) and (own.min() < -KEY_RANGE[d] or own.max() + 1 > KEY_RANGE[d]):
            raise ValueError("a sample's block or a + neighbour of it is out of key range: the truth does not model that")
        adds = self._adds(own, pkeys)
        if "no_mark" in self.variant:
            adds = ~np.isin(_keys(own), pkeys)
        added = own[adds]
        if "adds_neighbours" in self.variant:
            added = (added[:, None, :] + offs[None, :, :]).reshape(-1, d)
        added = np.unique(added, axis=0) if len(added) else np.zeros((0, d), np.int64)
        self.particle_blocks, self.sample_only = pb, added
        self.blocks = np.unique(np.concatenate([pb, added]), axis=0)
        # blocks whose membership depends on an undecided sample: added in some but not all of the ways to decide it
        sure, maybe = set(map(tuple, pb.tolist())), set(map(tuple, pb.tolist()))
        und = np.nonzero(self.und_cell)[0]
        sure |= set(map(tuple, own[adds & ~self.und_cell].tolist()))
        maybe |= set(map(tuple, own[adds & ~self.und_cell].tolist()))
        if len(und):
            always = None
            for combo in itertools.product((0, 1), repeat=d):
                cc = np.where(np.array(combo, bool)[None, :], self.cell_hi[und], self.cell_lo[und]) // bw
                a = self._adds(cc, pkeys)
                got = [tuple(b) if ok else None for b, ok in zip(cc.tolist(), a.tolist())]
                maybe |= {g for g in got if g is not None}
                always = got if always is None else [g if g == o else None for g, o in zip(got, always)]
            sure |= {g for g in always if g is not None}
        self.und_blocks = sorted(maybe - sure)
        akeys = _keys(self.blocks)
        self.ignored = ~np.isin(_keys(own), akeys)          # samples whose own block does not exist: in no node list
        return self.blocks

    # ------------------------------------------------------------------------------------------ votes
    def _pairs(self, cells, akeys):
        """every (sample, node) pair that could vote: (sample index, row of `cells`, nominal, certain)"""
        d, bw = self.d, T.bw_of(self.d)
        keys = T.node_key(cells)
        span = 2 if "stencil2" in self.variant else 3
        offs = np.array(list(itertools.product(range(4), repeat=d)), np.int64)            # from cell_lo
        node = self.cell_lo[:, None, :] + offs[None, :, :]                                   # [n, 4^D, d]
        rel = node - self.cell[:, None, :]
        nominal = np.all((rel >= 0) & (rel < span), axis=2)
        possible = np.all(node <= (self.cell_hi + span - 1)[:, None, :], axis=2)
        certain = np.all((node >= self.cell_hi[:, None, :]) & (node <= (self.cell_lo + span - 1)[:, None, :]), axis=2)
        # the sample's own block: active in the nominal way, in every way (certain), in some way (possible)
        own_nom = np.isin(_keys(self.cell // bw), akeys)
        own_all, own_any = np.ones(self.n, bool), np.zeros(self.n, bool)
        for combo in itertools.product((0, 1), repeat=d):
            a = np.isin(_keys(np.where(np.array(combo, bool)[None, :], self.cell_hi, self.cell_lo) // bw), akeys)
            own_all &= a
            own_any |= a
        if "no_own_block" in self.variant:
            own_nom[:] = own_all[:] = own_any[:] = True
        nominal &= own_nom[:, None]
        certain &= own_all[:, None]
        possible &= own_any[:, None]
        flat = node.reshape(-1, d)
        want = T.node_key(flat)
        j = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
        hit = (keys[j] == want) if len(keys) else np.zeros(len(want), bool)
        take = hit & possible.reshape(-1)
        self.n_node_block_missing = int((~hit & nominal.reshape(-1) & certain.reshape(-1)).sum())
        si = np.repeat(np.arange(self.n), offs.shape[0])[take]
        return si, j[take], nominal.reshape(-1)[take], certain.reshape(-1)[take]

    def _votes3(self, si, p, bp):
        """3D: (valid, valid_und, neg, neg_und, dist, b_dist) of every pair (sample si, node at p with bound bp)"""
        u, v = self.u, self.variant
        ia, ib, ic = (self.prim[si, k] for k in range(3))
        a, b, c = self.vw[ia], self.vw[ib], self.vw[ic]
        bvm = np.maximum(np.maximum(self.bv[ia], self.bv[ib]), self.bv[ic])
        ab, ac, bc = b - a, c - a, c - b
        ap, bq, cq = p - a, p - b, p - c
        lab, lac, lbc = _norm(ab), _norm(ac), _norm(bc)
        n = np.cross(ab, ac)
        if "reversed_normal" in v:
            n = -n
        nl = _norm(n)
        d00, d01, d11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
        d20, d21 = (ap * ab).sum(1), (ap * ac).sum(1)
        det = d00 * d11 - d01 * d01
        nv = d11 * d20 - d01 * d21              # |n|^2 times the coordinate of b (the edge ac opposite)
        nw = d00 * d21 - d01 * d20              # ... of c (the edge ab opposite)
        nu = det - nv - nw                      # ... of a (the edge bc opposite)
        exact = np.array([self.exact[int(k)] for k in self.col[si]], bool) if len(si) else np.zeros(0, bool)
        Ee = np.where(exact, 0.0, 2.0 * bvm + u * np.maximum(np.maximum(lab, lac), lbc))
        dn = Ee * (lab + lac) + np.where(exact, 0.0, C_CROSS * u * lab * lac)
        und = np.zeros(len(si), bool)
        clear_neg = np.zeros(len(si), bool)
        for num, le, q in ((nw, lab, ap), (nu, lbc, bq), (nv, lac, cq)):
            lq = _norm(q)
            E = np.where(exact, 0.0, bvm + bp + u * lq)
            dt = Ee * nl + le * dn + np.where(exact, 0.0, C_CROSS * u * le * nl)
            dd = dt * lq + le * nl * E + np.where(exact, 0.0, C_DOT[3] * u * le * nl * lq)
            und |= (np.abs(num) <= dd) & (dd > 0)
            clear_neg |= num < -dd
        # the area at 0: a zero area is decided where the cross product is one of exact zeros (all its products vanish) of
        # exact world vertices; otherwise an fp32 normal of rounding noise may point anywhere
        zero = nl == 0.0
        prod0 = np.all(np.stack([ab[:, 1] * ac[:, 2], ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0], ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1],
                                 ab[:, 1] * ac[:, 0]], 1) == 0.0, axis=1)
        zero_decided = zero & ((bvm == 0.0) & prod0 | exact)
        area_und = ~zero_decided & (((nl <= dn) & (dn > 0)) | zero)
        if "strict_edges" in v:
            inside = (nu > 0) & (nv > 0) & (nw > 0)
        else:
            inside = (nu >= 0) & (nv >= 0) & (nw >= 0)
        valid = ~zero & inside
        valid_und = (und & ~clear_neg & ~zero_decided) | area_und
        with np.errstate(divide="ignore", invalid="ignore"):
            sd = np.where(zero, 0.0, (n * ap).sum(1) / nl)
        lap = _norm(ap)
        E = np.where(exact, 0.0, bvm + bp + u * lap)
        with np.errstate(divide="ignore", invalid="ignore"):
            b_sd = np.where(zero, 0.0, dn * (lap + np.abs(sd)) / np.where(zero, 1.0, nl)) + E + np.where(exact, 0.0, (C_DOT[3] + 3.0) * u * lap)
        dist = np.abs(sd)
        # (exact decisions; the distance itself still goes through a square root and a division unless the normal is an axis)
        axis = (np.count_nonzero(n, axis=1) == 1)
        b_dist = b_sd + np.where(exact & axis, 0.0, 3.0 * u * dist)
        if "true_distance" in v or "no_validity" in v:
            td = _point_triangle(p, a, b, c)
            if "true_distance" in v:
                valid = ~zero
                dist = td
            else:
                valid = np.ones(len(si), bool)
        neg = sd < 0.0
        neg_und = (np.abs(sd) <= b_sd) & (b_sd > 0)
        self.on_edge = valid & ~valid_und & ((nu == 0) | (nv == 0) | (nw == 0))      # (decided: exact arithmetic)
        self.flat = zero_decided
        return valid, valid_und, neg, neg_und, dist, b_dist, exact & axis

    def _votes2(self, si, p, bp):
        u, v = self.u, self.variant
        ia, ib = self.prim[si, 0], self.prim[si, 1]
        a, b = self.vw[ia], self.vw[ib]
        bvm = np.maximum(self.bv[ia], self.bv[ib])
        ab, ap = b - a, p - a
        lab, lap = _norm(ab), _norm(ap)
        den = (ab * ab).sum(1)
        zero = den == 0.0
        dens = np.where(zero, 1.0, den)
        t = np.where(zero, 0.0, (ap * ab).sum(1) / dens)
        exact = np.array([self.exact[int(k)] for k in self.col[si]], bool) if len(si) else np.zeros(0, bool)
        Ee = np.where(exact, 0.0, 2.0 * bvm + u * lab)
        E = np.where(exact, 0.0, bvm + bp + u * lap)
        dnum = E * lab + lap * Ee + np.where(exact, 0.0, C_DOT[2] * u * lap * lab)
        dden = 2.0 * lab * Ee + np.where(exact, 0.0, C_DOT[2] * u * den)
        dt = (dnum + np.abs(t) * dden) / dens + np.where(exact, 0.0, u * np.abs(t))
        # the fp32 projection a + ab t differs from a when a component moves by more than half a spacing of a's
        sp_a, sp_b = (np.spacing(np.abs(x).astype(np.float32)).astype(np.float64) for x in (a, b))
        with np.errstate(divide="ignore", invalid="ignore"):
            thr_a = np.min(np.where(ab != 0, 0.5 * sp_a / np.abs(ab), np.inf), axis=1)
            thr_b = np.min(np.where(ab != 0, 0.5 * sp_b / np.abs(ab), np.inf), axis=1)
        if "endpoints_valid_2d" in v or "true_distance" in v:      # (the clamped projection counts wherever it falls)
            valid = ~zero
        else:
            valid = ~zero & (t > thr_a) & (1.0 - t > thr_b)
        near0 = ((np.abs(t) <= dt) & (dt > 0)) | ((t > 0) & (t <= dt + 2.0 * thr_a))
        near1 = ((np.abs(1.0 - t) <= dt) & (dt > 0)) | ((t < 1) & (1.0 - t <= dt + 2.0 * thr_b))
        len_und = zero & (bvm > 0)
        len_und |= ~zero & (lab <= Ee) & (Ee > 0)
        valid_und = ((near0 | near1) & ~zero) | len_und
        proj = a + ab * np.clip(t, 0.0, 1.0)[:, None]
        dp = p - proj
        dist = _norm(dp)
        nrm = np.stack([-ab[:, 1], ab[:, 0]], 1)
        if "reversed_normal" in v:
            nrm = -nrm
        labs = np.where(zero, 1.0, lab)
        sd = (dp * nrm).sum(1) / labs
        axis = np.count_nonzero(ab, axis=1) == 1
        # exact and along an axis: the component across the segment is exact, the one along it carries the rounding of t
        # and of the projection — unless |ab|^2 is a power of two: then t, the projection and the distance are exact too
        all_exact = exact & axis & (np.frexp(dens)[0] == 0.5)
        rnd = np.where(all_exact, 0.0, C_PROJ * u * (_norm(a) + lab))
        b_n = np.where(exact & axis, 0.0, E + Ee * lap / labs + rnd + u * dist)
        b_t = np.where(all_exact, 0.0, lab * dt + rnd)
        with np.errstate(divide="ignore", invalid="ignore"):
            b_dist = b_n + np.minimum(b_t, np.where(dist > 0, b_t * b_t / dist, b_t)) + np.where(exact & axis, 0.0, C_DIST * u * dist)
        neg = sd < 0.0
        neg_und = (np.abs(sd) <= b_n) & (b_n > 0)
        if "no_validity" in v:
            valid = np.ones(len(si), bool)
        self.on_edge = ~valid & ~valid_und & ~zero & ((t == 0.0) | (t == 1.0))         # (2D: on an end point, decided invalid)
        self.flat = zero & ~len_und
        return valid, valid_und, neg, neg_und, dist, b_dist, all_exact

    def fill(self, cells, nc, voter, inside, dist_c, b_c, aff_und, in_und, exact_c, dist_und):
        """the columns of the mesh colliders (ids < nc) at world cells [M, d] (sorted): what cdf_truth.NodeField merges"""
        d, bw = self.d, T.bw_of(self.d)
        cells = np.asarray(cells, np.int64)
        M = len(cells)
        akeys = _keys(self.blocks if self.blocks is not None else np.unique(cells // bw, axis=0))
        si, nj, nominal, certain = self._pairs(cells, akeys)
        p = cells[nj] * self.h
        bp = np.zeros(len(nj)) if T._pow2(self.h) else C_PT * self.u * _norm(p)
        valid, valid_und, neg, neg_und, dist, b, exact_d = (self._votes3 if d == 3 else self._votes2)(si, p, bp)
        col = self.col[si]
        self.pairs = dict(sample=si, node=nj, nominal=nominal, certain=certain, valid=valid, valid_und=valid_und, neg=neg,
                          neg_und=neg_und, dist=dist, col=col, on_edge=self.on_edge, flat=self.flat)
        for cid in np.unique(self.col):
            if cid >= nc:
                continue
            m = col == cid
            j = nj[m]
            vote = nominal[m] & valid[m]
            sure = certain[m] & valid[m] & ~valid_und[m]                     # a decided valid vote
            could = valid[m] | valid_und[m]                                  # (every pair here is a possible member)
            vt, ins = np.zeros(M, bool), np.zeros(M, bool)
            np.logical_or.at(vt, j[vote], True)
            sign_vote = vote & neg[m]
            if "sign_of_closest" in self.variant:
                dm = np.full(M, np.inf)
                np.minimum.at(dm, j[vote], dist[m][vote])
                sign_vote = vote & neg[m] & (dist[m] == dm[j])
            np.logical_or.at(ins, j[sign_vote], True)
            dec_set, can_set, dec_neg, can_neg = (np.zeros(M, bool) for _ in range(4))
            np.logical_or.at(dec_set, j[sure], True)
            np.logical_or.at(can_set, j[could], True)
            np.logical_or.at(dec_neg, j[sure & neg[m] & ~neg_und[m]], True)
            np.logical_or.at(can_neg, j[could & (neg[m] | neg_und[m])], True)
            dmin = np.full(M, np.inf)
            np.minimum.at(dmin, j[vote], dist[m][vote])
            bmax = np.zeros(M)
            np.maximum.at(bmax, j[vote], b[m][vote])
            near = vote & (dist[m] <= dmin[j] + 2.0 * bmax[j])
            bc = np.zeros(M)
            np.maximum.at(bc, j[near], b[m][near])
            # an undecided pair whose distance could undercut the minimum of the decided votes, within the two bounds
            dsure = np.full(M, np.inf)
            np.minimum.at(dsure, j[sure], dist[m][sure])
            open_ = could & ~sure
            du = np.zeros(M, bool)
            np.logical_or.at(du, j[open_ & (dist[m] - b[m] <= dsure[j] + bmax[j])], True)
            ex = np.ones(M, bool)
            np.logical_and.at(ex, j[vote], exact_d[m][vote])
            voter[:, cid], inside[:, cid] = vt, ins
            dist_c[:, cid], b_c[:, cid] = dmin, bc
            aff_und[:, cid], in_und[:, cid] = can_set & ~dec_set, can_neg & ~dec_neg
            exact_c[:, cid] = ex & bool(self.exact[int(cid)])
            dist_und[:, cid] = du


def _point_segment(p, a, b):
    ab, ap = b - a, p - a
    den = (ab * ab).sum(1)
    t = np.clip(np.where(den > 0, (ap * ab).sum(1) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
    return _norm(p - (a + ab * t[:, None]))


def _point_triangle(p, a, b, c):
    """distance of p [K, 3] to the triangles (a, b, c) [K, 3] each: the plane distance where the projection is inside, else the
    nearest edge"""
    ab, ac, ap = b - a, c - a, p - a
    n = np.cross(ab, ac)
    nl = _norm(n)
    d00, d01, d11 = (ab * ab).sum(1), (ab * ac).sum(1), (ac * ac).sum(1)
    d20, d21 = (ap * ab).sum(1), (ap * ac).sum(1)
    det = d00 * d11 - d01 * d01
    nv, nw = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20
    inside = (nl > 0) & (nv >= 0) & (nw >= 0) & (det - nv - nw >= 0)
    edge = np.minimum(np.minimum(_point_segment(p, a, b), _point_segment(p, b, c)), _point_segment(p, c, a))
    with np.errstate(divide="ignore", invalid="ignore"):
        plane = np.abs((n * ap).sum(1)) / nl
    return np.where(inside, plane, edge)


MESH_RIM = 0.5        # distance (in h) up to which a particle's three node layers hold two of the surface's three at least


def _valid_distance(c, x, d):
    """distance of points x to the nearest primitive of mesh record c on which their orthogonal projection falls (inf: none)"""
    vw = (c["scale"] * c["vertices"]) @ c["R"].T + c["trans"]
    out = np.full(len(x), np.inf)
    for prim in c["indices"]:
        a, b = vw[prim[0]], vw[prim[1]]
        if d == 2:
            ab, ap = b - a, x - a
            den = ab @ ab
            if den == 0:
                continue
            t = (ap @ ab) / den
            dist = _norm(ap - t[:, None] * ab)
            ok = (t > 0) & (t < 1)
        else:
            ab, ac, ap = b - a, vw[prim[2]] - a, x - a
            n = np.cross(ab, ac)
            nl = np.linalg.norm(n)
            if nl == 0:
                continue
            d00, d01, d11, d20, d21 = ab @ ab, ab @ ac, ac @ ac, ap @ ab, ap @ ac
            nv, nw = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20
            ok = (nv >= 0) & (nw >= 0) & (d00 * d11 - d01 * d01 - nv - nw >= 0)
            dist = np.abs(ap @ n) / nl
        out = np.where(ok, np.minimum(out, dist), out)
    return out


def rim_units(colliders, d, h):
    """for cdf_truth._static: the distance of positions to the nearest collider in units of its rim. A mesh reaches the
    three node layers of its samples' stencils and no farther, and only where a node's projection falls on a primitive:
    its rim is MESH_RIM h from the surface, measured to the primitives a position projects on; a position beside an open
    or convex edge, or one whose stencil hangs over it (a probe one h along an axis projects on no primitive), is at
    the rim whatever its distance; an analytic collider's rim is cdf_truth.RIM h."""
    cols = CT.colliders_of(colliders, d)

    def units(x):
        out = CT.signed_distance(cols, x, d) / (CT.RIM * h)
        for c in cols[:CT.MAXC]:
            if "vertices" in c:
                dv = _valid_distance(c, x, d)
                for k in range(d):
                    for sgn in (-h, h):
                        probe = x.copy()
                        probe[:, k] += sgn
                        dv = np.where(np.isfinite(_valid_distance(c, probe, d)), dv, np.inf)
                out = np.minimum(out, dv / (MESH_RIM * h))
        return out
    return units


MESH_RIM_KEEP = 0.004  # (cdf_truth.RIM_KEEP is 0.02 of a rim around a core 2 h thick and the inside; a sheet's core is 1 h thick and
                       # the same boxes hold a fifth of the core: the same weight of the rim in the undecided share)


def surface_distance(colliders, d):
    """world distance of positions to the nearest collider's surface (a mesh: to its primitives, edges and vertices included)"""
    cols = CT.colliders_of(colliders, d)

    def dist(x):
        out = np.abs(CT.signed_distance(cols, x, d))
        for c in cols[:CT.MAXC]:
            if "vertices" in c:
                vw = (c["scale"] * c["vertices"]) @ c["R"].T + c["trans"]
                for prim in c["indices"]:
                    pts = [np.broadcast_to(vw[k], x.shape) for k in prim]
                    out = np.minimum(out, _point_segment(x, *pts) if d == 2 else _point_triangle(x, *pts))
        return out
    return dist


def _static(d, h, rng, cols, boxes, n, near=None, **kw):
    """cdf_truth._static with the rim of mesh colliders. `near`: (distance in h, factor where every candidate is kept, factor where the rim is
    thinned out): `factor` times as many candidates are drawn and those within the distance of a collider's surface are kept, so that a sheet's thin core holds a few
    hundred particles where the rim is thinned out; n then bounds the particles, not the candidates (the scenes choose
    the factor so, and tests/test_mesh_truth.py asserts it)."""
    if h > CT.RIM_H:
        kw.setdefault("rim_keep", MESH_RIM_KEEP)
    if near is not None:
        reach, factor = near[0], near[1 if h <= CT.RIM_H else 2]
        dist, keep0 = surface_distance(cols, d), kw.pop("keep", None)
        kw["keep"] = lambda p: (dist(p) <= reach * h) & (True if keep0 is None else keep0(p))
        n = int(n * factor)
    return CT._static(d, h, rng, cols, boxes, n, rim_units=rim_units(cols, d, h), **kw)


def rigid_of(sc, poses=None, colliders=None, variant=()):
    """the Rigid of a scene (None without a mesh collider), at the uploaded poses or those of read_body_poses()"""
    from wgsparkl_amd.sampling import build_rigid_particles
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    cl = colliders or sc["colliders"]
    rb = build_rigid_particles(cl, d, float(h))
    if rb is None:
        return None
    return Rigid(rb, CT.colliders_of(cl, d, poses), d, h, variant=variant)


# ------------------------------------------------------------------------------------------------ scenes
def _sheet_mesh(d, h, ext=(9.0, 7.0)):
    """3D: two triangles sharing the diagonal of a rectangle in the local xz plane; 2D: six segments that zigzag"""
    from wgsparkl_amd.solver import Collider
    if d == 3:
        ex, ez = ext[0] * h, ext[1] * h
        v = np.array([[0, 0, 0], [ex, 0, 0], [0, 0, ez], [ex, 0, ez]], np.float32)
        return v, np.array([[0, 1, 2], [2, 1, 3]], np.uint32), Collider.trimesh
    v = np.array([[0, 0], [4.2, 0.6], [8.1, -0.4], [12.3, 0.2], [16.4, -0.5], [20.2, 0.4], [24.5, 0.0]], np.float32) * np.float32(h)
    return v, np.stack([np.arange(6), np.arange(1, 7)], 1).astype(np.uint32), Collider.polyline


def sheet(d, h, seed=20, **kw):
    """a two-triangle sheet (2D: a six-segment polyline), rotated by 33 degrees, scaled by 1.3, at non-round offsets;
    particles on both sides"""
    rng = np.random.default_rng(seed)
    v, idx, make = _sheet_mesh(d, h)
    c0 = np.array([5.37, 6.21, 5.13]) * h
    cols = [make(v, idx, CT._v(c0, d), rotation=CT._rot(d), scale=float(np.float32(1.3)))]
    return _static(d, h, rng, cols, [(c0 - np.array([5.5 if d == 3 else 2.5, 2.5, 2.5]) * h, c0 + np.array([11.0 if d == 3 else 29.0, 9.5 if d == 3 else 20.0, 12.5]) * h)], 3000 if d == 3 else 1500, near=(2.2, 4.4, 4.4), **kw)


ALIGNED_X = (0, 2, 10, 26, 34, 36, 37)


def _aligned_mesh(d, h, at):
    """the sheet in the node plane y = at[1], vertices on nodes (identity pose: exact when h is a power of two)"""
    from wgsparkl_amd.solver import Collider
    # (a second piece 2.75 h above the first, between node planes: there the cell of a sample depends on how x / h is rounded)
    if d == 3:
        v = np.array([[0, 0, 0], [6, 0, 0], [0, 0, 4], [6, 0, 4], [0, 2.75, 0], [6, 2.75, 0], [0, 2.75, 4], [6, 2.75, 4]], np.float32) * np.float32(h)
        return Collider.trimesh(v, np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 5, 7]], np.uint32), CT._v(np.asarray(at) * h, d), rotation=CT.ident(d))
    # (segments of 2 h, 8 h, 16 h, 8 h, 2 h, 1 h: |ab|^2 a power of two, so that t and the projection are exact as well)
    v = np.array([[x, 0] for x in ALIGNED_X] + [[2, 2.75], [10, 2.75]], np.float32) * np.float32(h)
    n = len(ALIGNED_X)
    idx = np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), [[n, n + 1]]]).astype(np.uint32)
    return Collider.polyline(v, idx, CT._v(np.asarray(at) * h, d), rotation=CT.ident(d))


def aligned(d, h, seed=21, **kw):
    """power-of-two h: exact arithmetic. The sheet lies in a node plane with its vertices on nodes: nodes on the plane
    (distance 0, positive sign), nodes whose projection is on the shared diagonal and on the outer edges (valid; 2D: on a
    shared vertex, which is an end point of both segments: no vote), nodes one step outside (no vote)"""
    rng = np.random.default_rng(seed)
    at = np.array([2.0, 4.0, 2.0])
    cols = [_aligned_mesh(d, h, at)]
    lo, hi = (at - np.array([1.9, 1.3, 1.9])) * h, (at + np.array([7.9 if d == 3 else 38.9, 4.0, 5.9])) * h
    if d == 2:      # (the node columns over the polyline's vertices hold no vote: a stencil that includes one fits two columns)
        kw.setdefault("keep", lambda p: np.all(np.abs(p[:, :1] / h - (at[0] + np.array(ALIGNED_X, np.float64))[None, :]) > 1.6, axis=1)
                      | (p[:, 1] / h - at[1] < -1.6) | (p[:, 1] / h - at[1] > 4.4))
    return _static(d, h, rng, cols, [(lo, hi)], 3000 if d == 3 else 1500, near=(2.2, 4.0, 4.0), **kw)


def _solid_mesh(d, h, k):
    if d == 3 and k == 0:       # octahedron
        v = np.array([[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]], np.float32)
        i = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)
    elif d == 3:                # square pyramid
        v = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2], [0, 3, 0]], np.float32)
        i = np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], np.uint32)
    elif k == 0:                # a hexagon, closed
        v = np.array([[2, 0], [1, 1.7], [-1, 1.7], [-2, 0], [-1, -1.7], [1, -1.7]], np.float32)
        i = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 0]], np.uint32)
    else:                       # a closed thin plate (0.9 h thick at the scale below): both faces reach the nodes around it
        # (wound clockwise: the left normals point outwards, so a node above it takes a positive vote from the near face and a
        # negative one from the far face; the hexagon is wound the other way)
        v = np.array([[-3, -0.2], [3, -0.2], [3, 0.2], [-3, 0.2]], np.float32)
        i = np.array([[1, 0], [2, 1], [3, 2], [0, 3]], np.uint32)
    return v * np.float32((1.1 if d == 3 else 2.3) * h), i


def solid(d, h, seed=22, **kw):
    """the octahedron and the square pyramid of test_rigid_particles.py (2D: a closed hexagon and a closed thin plate), rotated,
    with particles around and inside: nodes with votes of both signs from different faces, nodes beyond a convex edge with
    none"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    make = Collider.trimesh if d == 3 else Collider.polyline
    c0 = np.array([5.37, 5.21, 5.13]) * h
    c0 = c0 + (np.array([3.0, 3.0, 0.0]) * h if d == 2 else 0.0)
    c1 = c0 + np.array([6.6 if d == 3 else 13.6, 0.4, 0.3]) * h
    cols = [make(*_solid_mesh(d, h, 0), CT._v(c0, d), rotation=CT._rot(d, 21.0)),
            make(*_solid_mesh(d, h, 1), CT._v(c1, d), rotation=CT._rot(d, -14.0))]
    if d == 2:      # (the wedges beyond the corners of one convex outline hold pi 1.5^2 = 7 nodes whatever its shape: a third outline)
        sq = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float32) * np.float32(2.3 * h)
        cols.append(make(sq, np.array([[0, 1], [1, 2], [2, 3], [3, 0]], np.uint32), CT._v(c0 + np.array([6.8, 7.6, 0.0]) * h, d), rotation=CT._rot(d, 38.0)))
    return _static(d, h, rng, cols, [(c0 - (3.4 if d == 3 else 5.6) * h, c1 + np.array([3.4 if d == 3 else 7.6, 4.6 if d == 3 else 9.6, 3.4]) * h)], 3000 if d == 3 else 1500, near=(2.2, 1.6, 4.0), **kw)


def heightfield(d, h, seed=23, **kw):
    """a 7 x 7 undulating heightfield under a bed (2D: a fifteen-vertex undulating polyline): many small triangles, shared edges,
    several samples per node"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    c0 = np.array([6.37, 3.21, 6.13]) * h
    if d == 3:
        ii, jj = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
        hts = (0.5 * np.sin(0.9 * ii) * np.cos(0.7 * jj)).astype(np.float32)
        cols = [Collider.heightfield(hts, (float(np.float32(9.0 * h)), float(np.float32(1.2 * h)), float(np.float32(9.0 * h))), CT._v(c0, d),
                                     rotation=_quat_small())]
        lo, hi = c0 - np.array([4.0, 1.8, 4.0]) * h, c0 + np.array([4.0, 2.8, 4.0]) * h
    else:
        x = np.arange(15) * 1.5 - 4.5
        v = np.stack([x, 0.6 * np.sin(0.9 * np.arange(15))], 1).astype(np.float32) * np.float32(h)
        cols = [Collider.polyline(v, np.stack([np.arange(14), np.arange(1, 15)], 1).astype(np.uint32), CT._v(c0, d),
                                  rotation=(float(np.float32(math.radians(4.0))),))]
        lo, hi = c0 - np.array([4.0, 1.8, 0.0]) * h, c0 + np.array([16.0, 3.8, 0.0]) * h
    return _static(d, h, rng, cols, [(lo, hi)], 3000 if d == 3 else 1500, **kw)


def _quat_small():
    return CT._quat((3.0, 1.0, 2.0), 4.0)


def mixed(d, h, seed=24, mesh_first=False, **kw):
    """a cuboid whose top face coincides with an `aligned` sheet that extends past it on +x: where both reach a node they tie
    exactly (power-of-two h, 3D) and the lowest id wins, beside the cuboid the mesh alone votes, below its top the cuboid is
    nearer at its sides; both colliders' bits in one word. `mesh_first`: the other id order"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    at = np.array([2.0, 4.0, 2.0])
    mesh = _aligned_mesh(d, h, at)
    he = np.array([2.0 if d == 3 else 12.0, 1.0, 2.0])
    box = Collider.cuboid(CT._v(he * h, d), CT._v((at + np.array([he[0], -1.0, 2.0])) * h, d), rotation=CT.ident(d))
    cols = [mesh, box] if mesh_first else [box, mesh]
    lo, hi = (at - np.array([1.9, 3.3, 1.9])) * h, (at + np.array([7.9 if d == 3 else 38.9, 4.0, 5.9])) * h
    return _static(d, h, rng, cols, [(lo, hi)], 3000 if d == 3 else 1500, **kw)


def mixed_mesh_first(d, h, seed=24, **kw):
    return mixed(d, h, seed=seed, mesh_first=True, **kw)


def slot15(d, h, seed=25, **kw):
    """fifteen small balls and a sheet as the sixteenth collider: bits 15 and 31"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    cols = [Collider.ball(float(np.float32(0.45 * h)), CT._v(np.array([1.31 + 2.5 * i, 2.23, 2.17]) * h, d)) for i in range(15)]
    v, idx, make = _sheet_mesh(d, h)
    c0 = np.array([3.37, 5.21, 0.63]) * h
    cols.append(make(v, idx, CT._v(c0, d), rotation=CT._rot(d, 11.0), scale=float(np.float32(1.3))))
    boxes = [(np.array([-1.4, -0.4, -0.4]) * h, np.array([37.9, 4.9, 4.9]) * h), (c0 - 2.0 * h, c0 + np.array([13.5 if d == 3 else 33.5, 5.0 if d == 3 else 9.0, 11.0]) * h)]
    return _static(d, h, rng, cols, boxes, 3000 if d == 3 else 1500, **kw)


def degenerate(d, h, seed=26, **kw):
    """zero-area triangles (collinear along an axis, a repeated vertex), a triangle smaller than a cell (2D: a zero-length
    segment and one shorter than a cell) next to sound primitives; identity pose at translation 0, so that the world
    vertices are the local ones and a zero area is one of exact zeros: none of them votes, the sound ones do"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    if d == 3:
        y = 4.75
        v = np.array([[2.37, y, 2.13], [8.37, y, 2.13], [2.37, y, 7.13], [8.37, y, 7.13],   # 0-3: the sound sheet
                      [5, y + 1.5, 2], [8, y + 1.5, 2], [6.5, y + 1.5, 2],     # 4-6: collinear along x
                      [3.37, y + 1.5, 5.13],                                   # 7: with 2 twice: a repeated vertex
                      [4.3, y + 1.25, 4.1], [4.7, y + 1.25, 4.2], [4.4, y + 1.25, 4.6]], np.float32) * np.float32(h)   # 8-10: smaller than a cell
        idx = np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6], [2, 2, 7], [8, 9, 10]], np.uint32)
        cols = [Collider.trimesh(v, idx, (0.0,) * 3, rotation=CT.ident(3))]
        lo, hi = np.array([1.0, y - 1.3, 1.0]) * h, np.array([9.5, y + 2.7, 8.5]) * h
    else:
        y = 4.25
        v = np.array([[2, y], [9, y + 0.4], [9, y + 0.4], [16, y], [16.3, y + 0.2], [23, y - 0.1], [3.4, y + 1.3], [19.6, y + 1.2]], np.float32) * np.float32(h)
        idx = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [6, 6], [7, 7]], np.uint32)
        cols = [Collider.polyline(v, idx, (0.0,) * 2, rotation=CT.ident(2))]
        lo, hi = np.array([0.5, y - 2.5]) * h, np.array([24.5, y + 2.8]) * h
    return _static(d, h, rng, cols, [(lo, hi)], 3000 if d == 3 else 1500, near=(2.2, 1.05, 4.0), **kw)


LONELY_COLUMNS = (1, 4, 7)      # the blocks along x that hold particles


def lonely(d, h, seed=27, **kw):
    """Sheets that extend well past the particles, one in every other row of blocks (two cells under the row's top), through
    three columns of particles one block wide with two blocks between them. Of those two the first is the + neighbour of
    a column's block; the second, like the block before the first column, holds no particle and is no + neighbour of one
    that does, while its own + neighbour is: it exists only where a sample adds it, once per sheet (3D: and per block
    along z), and its nodes carry votes. Past the last column the samples have no block anywhere near and are ignored.
    The top node of a sample's stencil lies in the row above, which exists only over the columns. A second piece lower
    down in the first row ends 0.3 h into the block before the first column: its samples lie in blocks that do not
    exist, and the node column at the start of that block projects on it but receives no vote — unless a sample whose
    own block is missing is taken for one that votes."""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    bw = T.bw_of(d)
    rows = range(2, 18 if d == 2 else 10, 2)
    c0 = np.array([-2.0 * bw + 0.37, (rows[0] + 1.0) * bw - 1.29, -2.0 * bw + 0.13]) * h
    yb, xa, xb = -(bw - 1.59), 0.5 * bw, 2.0 * bw - 0.07
    length, depth = 11 * bw, 6 * bw
    vtx, idx = [], []
    for r in rows:
        y = (r - rows[0]) * bw
        k = len(vtx)
        if d == 3:
            vtx += [[0, y, 0], [length, y, 0], [0, y, depth], [length, y, depth]]
            idx += [[k, k + 1, k + 2], [k + 2, k + 1, k + 3]]
        else:
            vtx += [[0, y], [3 * bw, y + 0.2], [6 * bw, y - 0.15], [length, y + 0.1]]
            idx += [[k, k + 1], [k + 1, k + 2], [k + 2, k + 3]]
    k = len(vtx)
    if d == 3:
        vtx += [[xa, yb, 3.2 * bw], [xb, yb, 3.2 * bw], [xa, yb, 5.0 * bw], [xb, yb, 5.0 * bw]]
        idx += [[k, k + 1, k + 2], [k + 2, k + 1, k + 3]]
        make, rot = Collider.trimesh, CT._quat((3.0, 1.0, 2.0), 0.3)
    else:
        vtx += [[xa, yb], [xb, yb]]
        idx += [[k, k + 1]]
        make, rot = Collider.polyline, (float(np.float32(math.radians(0.2))),)
    cols = [make(np.array(vtx, np.float32) * np.float32(h), np.array(idx, np.uint32), CT._v(c0, d), rotation=rot)]
    # (a position x lies in cell rint(x / h) - 1: the boxes start 1.2 h or more past a block's first node)
    boxes = [(np.array([(c + 0.3) * bw, rows[0] * bw + 1.3, 1.3 * bw]) * h, np.array([(c + 0.95) * bw, (rows[-1] + 1) * bw - 0.3, 3.4 * bw]) * h)
             for c in LONELY_COLUMNS]
    return _static(d, h, rng, cols, boxes, 2990 if d == 3 else 1490, **kw)


def far_mesh(sc):
    """the scene plus a small mesh collider more than 4 blocks from every particle: it adds no block and leaves no bit"""
    from wgsparkl_amd.solver import Collider
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    at = tuple(float(np.float32(v)) for v in ps.pos.max(0) + 7 * T.bw_of(d) * h)
    if d == 3:
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [1, 0, 1]], np.float32) * np.float32(2 * h)
        mesh = Collider.trimesh(v, np.array([[0, 1, 2], [2, 1, 3]]), at)
    else:
        v = np.array([[0, 0], [1, 0.2], [2, 0]], np.float32) * np.float32(2 * h)
        mesh = Collider.polyline(v, np.array([[0, 1], [1, 2]]), at)
    out = dict(sc)
    out["colliders"] = list(sc["colliders"]) + [mesh]
    return out


SCENES = dict(sheet=sheet, aligned=aligned, solid=solid, heightfield=heightfield, mixed=mixed, mixed_mesh_first=mixed_mesh_first,
              slot15=slot15, degenerate=degenerate, lonely=lonely)
POW2_ONLY = ("aligned", "mixed", "mixed_mesh_first")
CASES = [(name, d, h) for name in SCENES for d in (2, 3) for h in CT.HS if T._pow2(h) or name not in POW2_ONLY]


def counts(rg: Rigid, nf):
    """how often a scene reaches the cases the scenes are named for (decided instances only)"""
    P = rg.pairs
    M = len(nf.cells)
    dec = P["certain"] & ~P["valid_und"]
    mesh_cols = [int(c) for c in np.unique(rg.col) if c < nf.voter.shape[1]]
    out = {}
    # nodes exactly on the plane / line of a valid vote: distance 0, positive sign
    on = dec & P["valid"] & (P["dist"] == 0.0) & ~P["neg"] & ~P["neg_und"]
    out["on_plane"] = len(np.unique(P["node"][on]))
    out["on_edge"] = len(np.unique(P["node"][dec & P["on_edge"]]))
    out["flat_pairs"] = int((dec & P["flat"] & ~P["valid"]).sum())
    okp = dec & P["valid"]
    out["node_block_missing"] = rg.n_node_block_missing
    out["positive"], out["negative"] = int(((nf.aff & 0xffff) != 0).sum() - ((nf.aff >> np.uint32(16)) != 0).sum()), int(((nf.aff >> np.uint32(16)) != 0).sum())
    out["two_colliders"] = int((nf.voter.sum(1) >= 2).sum())
    out["multi_vote"] = int((np.bincount(P["node"][okp], minlength=M) >= 2).sum())
    pos_n = np.zeros(M, bool)
    ok = dec & P["valid"] & ~P["neg_und"]
    for c in mesh_cols:
        m = ok & (P["col"] == c)
        a, b = np.zeros(M, bool), np.zeros(M, bool)
        a[P["node"][m & ~P["neg"]]] = True
        b[P["node"][m & P["neg"]]] = True
        pos_n |= a & b
    out["two_sign"] = int(pos_n.sum())
    # nodes in the stencil of a sample, every pair of which is decided invalid: beyond an edge
    reach, any_valid = np.zeros(M, bool), np.zeros(M, bool)
    reach[P["node"][P["nominal"]]] = True
    any_valid[P["node"][P["valid"] | P["valid_und"]]] = True
    out["no_vote"] = int((reach & ~any_valid).sum())
    first = nf.closest.astype(np.int64)
    vt = nf.voter
    has = first < vt.shape[1]
    tie = np.zeros(M, bool)
    if vt.shape[1] > 1:
        eq = vt & (nf.dist_c == nf.dist[:, None])
        tie = has & (eq.sum(1) >= 2) & ~nf.und_tie & ~nf.und_dist
    out["exact_tie"] = int(tie.sum())
    out["bit31"] = int((((nf.aff >> np.uint32(31)) & 1).astype(bool) & (((nf.und_bits >> np.uint32(31)) & 1) == 0)).sum())
    out["sample_only_blocks"] = len(rg.sample_only)
    nodes_of_added = np.isin(_keys(nf.cells // T.bw_of(rg.d)), _keys(rg.sample_only)) if len(rg.sample_only) else np.zeros(M, bool)
    out["sample_only_nodes_with_votes"] = int((nodes_of_added & (nf.aff != 0) & (nf.und_bits == 0)).sum())
    out["ignored_samples"] = int((rg.ignored & ~rg.und_cell).sum())
    return out
