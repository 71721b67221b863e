"""fp64 truth for the per-particle constitutive arithmetic of the G2P (wgsparkl_amd/csrc/device_math.h): the SVD, the
Kirchhoff stresses and the Drucker-Prager projection, computed from the SAME fp32 inputs the kernels see, and the a-priori
error bounds the HIP results are held to. Shared by tests/test_gpu_devmath.py (the device functions one lane per matrix)
and tests/test_gpu_constitutive.py (the same arithmetic inside the product's G2P kernels).

Two independent routes to the truth: numpy's LAPACK SVD (the convention of oracle/np_oracle.py: proper rotations, the sign
on the smallest singular value) and the C oracle's fp64 one-sided Jacobi (oracle/mpm_oracle.c orc_svd / orc_kirchoff_stress
/ orc_drucker_prager_project through oracle/orc.py). The two must agree to fp64 round-off before either is used.

The stress and Drucker-Prager truth is restated here rather than called from oracle/np_oracle.py because the tests need
more than the branch the reference takes: the decision quantities (trace, gamma, |dev|), the fp32 band around each
threshold and the outcome of EVERY branch, for the particles a correct fp32 evaluation may send either way. Where the
decision is clear it is checked against np_oracle (tests/test_gpu_devmath.py test_catalogue_and_truths_agree).

Every bound is C * u * scale with u = 2^-24, C fixed below and the scale written next to each check; every check is
reported through helpers.report_margin (measured / bound, so 1.0 is the edge)."""
import itertools

import numpy as np

from helpers import report_margin
from oracle.np_oracle import mat64 as mat, unmat

U32 = 2.0 ** -24          # unit round-off of fp32
CUTOFF = 1.0e-7           # device_math.h svd: a singular value at or below CUTOFF * s_max is set to 0 (its U column rebuilt)
NH_CLAMP = 1.0e-10        # device_math.h kirchoff_neo_hookean: J = max(det F, 1e-10)

# a-priori constants (multiples of u); derivations in the comments of the checks that use them
C_REC = 64        # reconstruction: ~15 fp32 rotations of columns, each ~2 u of the column pair's norm
C_ORTH = 64       # orthogonality / determinant of U and V (c^2 + s^2 off unit length by ~1 ulp per rotation)
C_SV = 32         # singular values (the column norms of the rotated matrix)
C_VEC = 64        # singular vectors, times s_max / gap
C_TAU = 64        # Kirchhoff stress, normwise
C_DP = 128        # Drucker-Prager outputs (log, exp, sin on top of the SVD)
C_DEC = 64        # width of the band around a discrete threshold inside which fp32 and fp64 may decide differently
VEC_MAX_BOUND = 0.25   # singular vectors are compared only where the gap makes their bound smaller than this


def rotations(rng, n, d):
    q, r = np.linalg.qr(rng.normal(size=(n, d, d)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1.0
    return q


def _usv(rng, s):
    s = np.asarray(s, np.float64)
    n, d = s.shape
    return rotations(rng, n, d) @ (s[:, :, None] * np.transpose(rotations(rng, n, d), (0, 2, 1)))


def catalogue(dim, seed=0, per=48):
    """{family: fp32 [n, d*d] column-major}. Hard deformations for the per-particle arithmetic: inverted, clustered,
    rank-deficient, badly conditioned, far from F = I in scale, and the structured matrices on which a Jacobi rotation
    is skipped (gamma == 0)."""
    rng = np.random.default_rng(9000 + 17 * seed + dim)
    d = dim
    fam = {}
    fam["well_conditioned"] = _usv(rng, np.exp(rng.uniform(np.log(0.2), np.log(5.0), (per, d))))
    s = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (per, d)))
    s = np.sort(s, 1)[:, ::-1].copy()
    s[:, -1] = np.minimum(s[:, -1], 0.8 * s[:, -2])            # a distinct smallest |s| ...
    s[:, -1] *= -1.0                                             # ... carrying the sign: det F < 0
    fam["inverted_distinct"] = _usv(rng, s)
    if d == 3:
        s = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (per, 3)))
        s[:, 2] = s[:, 1] = np.minimum(s[:, 1], s[:, 0])        # the smallest |s| twice ...
        s[:, 2] *= -1.0                                          # ... one of them negative
    else:
        s = np.tile(np.exp(rng.uniform(np.log(0.3), np.log(3.0), (per, 1))), (1, 2))
        s[:, 1] *= -1.0
    fam["inverted_tied"] = _usv(rng, s)
    for delta in (0.0, 1e-7, 1e-6, 1e-4):
        base = np.arange(d, dtype=np.float64) * delta + 1.0
        c = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (per // 4, 1)))
        fam[f"clustered_{delta:g}"] = _usv(rng, base[None, :] * c)
    c = rng.uniform(0.3, 3.0, (8, 1, 1))
    eye = np.eye(d)[None]
    R = rotations(rng, 8, d)
    perms = np.array([np.eye(d)[list(p)] for p in itertools.permutations(range(d))])
    diag = np.stack([np.diag(v) for v in rng.uniform(0.2, 4.0, (8, d)) * rng.choice([-1.0, 1.0], (8, d))])
    shear = []
    for a in range(d):
        for b in range(d):
            if a != b:
                m = np.eye(d)
                m[a, b] = rng.uniform(-2.0, 2.0)
                shear.append(m)
    fam["structured"] = np.concatenate([R, eye, c * eye, c * R, perms, diag, np.stack(shear), 1e-3 * R[:2], 1e3 * R[:2]])
    rk = []
    for r in range(d):                                           # rank r: singular values (s, ..., 0, ..., 0)
        s = np.zeros((per // 4, d))
        s[:, :r] = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (per // 4, r)))
        rk.append(_usv(rng, s))
    fam["rank_deficient"] = np.concatenate(rk)
    cut = []
    for f in (0.5, 0.9, 1.1, 2.0, 10.0):                        # s_min / s_max below and above the 1e-7 cutoff
        s = np.exp(rng.uniform(np.log(0.5), np.log(2.0), (per // 8, d)))
        s[:, 0] = 1.0
        s[:, -1] = f * CUTOFF
        cut.append(_usv(rng, s))
        if d == 3:                                               # two of them vanishing together (the nbad = 2 rebuild)
            s2 = s.copy()
            s2[:, 1] = f * CUTOFF * 0.5
            cut.append(_usv(rng, s2))
    fam["near_cutoff"] = np.concatenate(cut)
    cond = []
    for k in (1e2, 1e3, 1e4, 1e5, 1e6):
        s = np.ones((per // 8, d))
        s[:, -1] = 1.0 / k
        if d == 3:
            s[:, 1] = np.exp(rng.uniform(np.log(1.0 / k), 0.0, per // 8))
        cond.append(_usv(rng, s) * rng.choice([-1.0, 1.0], (per // 8, 1, 1)))
    fam["ill_conditioned"] = np.concatenate(cond)
    for sc in (1e-3, 1e3):
        fam[f"scale_{sc:g}"] = sc * _usv(rng, np.exp(rng.uniform(np.log(0.3), np.log(3.0), (per // 4, d))))
    return {k: unmat(v).astype(np.float32) for k, v in fam.items()}


def dp_catalogue(dim, rng):
    """(family -> fp32 F) for the projection: det F > 0 and s_min / s_max above 1e-4 (below, log s carries the SVD's
    u * s_max / s_min and at the cutoff log 0 = -inf: not a deformation a grain survives), with pure compression
    c I (the exact-equality branch all_zero), pure dilation, shear and the catalogue's positive families."""
    d = dim
    cat = catalogue(dim, seed=1)
    out = {}
    for fam, F32 in cat.items():
        if fam.startswith("inverted") or fam in ("rank_deficient", "near_cutoff"):
            continue
        a, smax, _ = sv_stats(svd_lapack(F32)[1])
        keep = (np.linalg.det(mat(F32, d)) > 0) & (a[:, -1] > 1e-4 * smax)
        out[fam] = F32[keep]
    c = np.linspace(0.5, 0.999, 96)
    eye = np.eye(d).reshape(-1)
    out["pure_compression"] = (c[:, None] * eye[None]).astype(np.float32)
    out["pure_dilation"] = ((1.0 + c[:, None] * 0.2) * eye[None]).astype(np.float32)
    R = rotations(rng, 96, d)
    out["compressed_rotated"] = unmat(c[:, None, None] * R).astype(np.float32)
    sc = np.exp(rng.normal(0.0, 0.15, (96, d)))
    out["compressed_sheared"] = unmat(rotations(rng, 96, d) @ (0.8 * sc[:, :, None] * np.transpose(rotations(rng, 96, d), (0, 2, 1)))).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ truth: SVD
def svd_lapack(F32):
    """fp64 SVD of the fp32 matrices (LAPACK), in the shipped convention: U, V proper rotations, the sign on the
    smallest singular value. -> (U [n,d,d], s [n,d] descending by |s|, V [n,d,d])"""
    F = mat(F32, int(round(np.sqrt(np.asarray(F32).shape[1]))))
    U, s, Vt = np.linalg.svd(F)
    U, s, V = U.copy(), s.copy(), np.transpose(Vt, (0, 2, 1)).copy()
    fu = np.linalg.det(U) < 0
    fv = np.linalg.det(V) < 0
    U[fu, :, -1] *= -1.0
    V[fv, :, -1] *= -1.0
    s[fu != fv, -1] *= -1.0
    return U, s, V


def svd_c_oracle(orc64, F32):
    d = orc64.dim
    out = [orc64.svd(f.astype(np.float64)) for f in np.asarray(F32)]
    U = np.stack([mat(u[None], d)[0] for u, _, _ in out])
    s = np.stack([s for _, s, _ in out])
    V = np.stack([mat(vt[None], d)[0].T for _, _, vt in out])
    return U, s, V


def sv_stats(s):
    """sorted |s| descending, s_max, the gap of every sorted value to its nearest neighbour"""
    a = np.sort(np.abs(s), 1)[:, ::-1]
    smax = a[:, 0]
    gaps = np.full(a.shape, np.inf)
    for i in range(a.shape[1]):
        for j in range(a.shape[1]):
            if i != j:
                gaps[:, i] = np.minimum(gaps[:, i], np.abs(a[:, i] - a[:, j]))
    return a, smax, gaps


def kappa_kept(abs_s):
    """s_max / the smallest singular value the fp32 SVD keeps (above the cutoff, with a factor 2 of margin): the
    amplification of a column's absolute round-off (~u s_max) into the direction of that column of U = F V / s."""
    smax = abs_s[:, 0]
    kept = np.where(abs_s > 2.0 * CUTOFF * smax[:, None], abs_s, np.inf)
    smin = kept.min(1)
    return np.where(np.isfinite(smin) & (smin > 0), smax / np.where(smin > 0, smin, 1.0), 1.0)


def check_svd(tag, F32, U, S, V, truth, sign_rows=None):
    """Per-matrix checks of a device SVD against the fp64 truth (U, s, V) of the same fp32 input. Returns the list of
    failures (empty = pass); every bound is reported."""
    d = U.shape[1]
    F = mat(F32, d)
    Ut, st, Vt_ = truth
    abs_t, smax, gaps = sv_stats(st)
    kap = kappa_kept(abs_t)
    fn = np.linalg.norm(F, axis=(1, 2))
    fails = []
    eye = np.eye(d)

    def bound(name, val, b, extra=None):
        val, b = np.asarray(val, np.float64), np.asarray(b, np.float64)
        bad = ~(val <= b)
        r = np.where(b > 0, val / np.where(b > 0, b, 1.0), np.where(val > 0, np.inf, 0.0))
        worst = int(np.nanargmax(np.where(np.isfinite(r), r, 1e300))) if r.size else 0
        report_margin(f"{tag}: {name}", float(val.flat[worst]) if r.size else 0.0, float(b.flat[worst]) if r.size else 0.0,
                      n=int(val.size), failures=int(bad.sum()))
        if bad.any():
            i = int(np.argmax(bad))
            fails.append(f"{tag}: {name}: {int(bad.sum())} of {bad.size} over the bound (first #{i}: {float(val.flat[i]):.3e} > "
                         f"{float(b.flat[i]):.3e})")

    rec = U @ (S[:, :, None] * np.transpose(V, (0, 2, 1)))
    # reconstruction: ~15 rotations of fp32 columns, each off by ~u times the pair's norm
    bound("reconstruction |U S V^T - F| / (u |F|)", np.linalg.norm(rec - F, axis=(1, 2)), C_REC * U32 * np.maximum(fn, 1e-300))
    # V is a product of rotations only; U's column c is a rotated column of F over its norm s_c: its absolute round-off
    # (~u s_max) becomes u * s_max / s_c in direction — bounded by kappa_kept (rebuilt columns are orthogonal by construction)
    bound("orthogonality |V^T V - I|", np.linalg.norm(np.transpose(V, (0, 2, 1)) @ V - eye, axis=(1, 2)),
          np.full(len(F), C_ORTH * U32))
    bound("orthogonality |U^T U - I| (scale s_max / s_kept_min)", np.linalg.norm(np.transpose(U, (0, 2, 1)) @ U - eye, axis=(1, 2)),
          C_ORTH * U32 * kap)
    bound("proper rotation |det V - 1|", np.abs(np.linalg.det(V) - 1.0), np.full(len(F), C_ORTH * U32))
    bound("proper rotation |det U - 1| (scale s_max / s_kept_min)", np.abs(np.linalg.det(U) - 1.0), C_ORTH * U32 * kap)
    a = np.sort(np.abs(S), 1)[:, ::-1]
    bound("singular values |s - s64| / (u s_max)", np.abs(a - abs_t).max(1), C_SV * U32 * smax)
    # sign convention: exactly one negative value iff det F < 0, on the smallest |s| — decided only where the smallest
    # singular value is clear of the round-off of the values themselves
    sv_err = C_SV * U32 * smax
    clear = abs_t[:, -1] > 2.0 * sv_err
    neg_t = st.min(1) < 0
    nneg = (S < 0).sum(1)
    want = np.where(neg_t, 1, 0)
    wrong = clear & (nneg != want)
    on_small = np.abs(np.where(S < 0, S, np.inf)).min(1)
    wrong |= clear & neg_t & ~(on_small <= np.abs(S).min(1) + sv_err)
    report_margin(f"{tag}: sign convention violations", float(wrong.sum()), 0.0, checked=int(clear.sum()))
    if wrong.any():
        i = int(np.argmax(wrong))
        fails.append(f"{tag}: sign convention wrong for {int(wrong.sum())} of {int(clear.sum())} (first #{i}: s = {S[i]}, truth {st[i]})")
    # singular vectors, where the gap to the neighbouring value permits: angle ~ u s_max / gap; U's also ~ u s_max / s
    order_g = np.argsort(-np.abs(S), 1)
    order_t = np.argsort(-np.abs(st), 1)
    vb, vv, ub, uv = [], [], [], []
    for i in range(d):
        gi = np.take_along_axis(V, order_g[:, None, i:i + 1], 2)[:, :, 0]
        ti = np.take_along_axis(Vt_, order_t[:, None, i:i + 1], 2)[:, :, 0]
        gu = np.take_along_axis(U, order_g[:, None, i:i + 1], 2)[:, :, 0]
        tu = np.take_along_axis(Ut, order_t[:, None, i:i + 1], 2)[:, :, 0]
        bv = C_VEC * U32 * smax / np.maximum(gaps[:, i], 1e-300)
        bu = C_VEC * U32 * smax / np.maximum(np.minimum(gaps[:, i], abs_t[:, i]), 1e-300)
        ev = np.minimum(np.linalg.norm(gi - ti, axis=1), np.linalg.norm(gi + ti, axis=1))
        eu = np.minimum(np.linalg.norm(gu - tu, axis=1), np.linalg.norm(gu + tu, axis=1))
        mv, mu_ = bv < VEC_MAX_BOUND, bu < VEC_MAX_BOUND
        vb.append(bv[mv]); vv.append(ev[mv]); ub.append(bu[mu_]); uv.append(eu[mu_])
    bound("right singular vectors (scale s_max / gap)", np.concatenate(vv), np.concatenate(vb))
    bound("left singular vectors (scale s_max / min(gap, s))", np.concatenate(uv), np.concatenate(ub))
    return fails


# ------------------------------------------------------------------------------------------------ truth: stress
def tau_corotated64(F, lam, mu, U, s):
    """tau = 2 mu (F F^T - U S U^T) + lambda (J - 1) J I, from an fp64 SVD of F"""
    d = F.shape[1]
    J = np.prod(s, 1)
    return 2.0 * mu[:, None, None] * (F @ np.transpose(F, (0, 2, 1)) - (U * s[:, None, :]) @ np.transpose(U, (0, 2, 1))) + \
        (lam * (J - 1.0) * J)[:, None, None] * np.eye(d)


def tau_neo_hookean64(F, lam, mu):
    d = F.shape[1]
    j = np.maximum(np.linalg.det(F), NH_CLAMP)
    return mu[:, None, None] * (F @ np.transpose(F, (0, 2, 1))) + (lam * np.log(j) - mu)[:, None, None] * np.eye(d)


def tau_scales(model, F, lam, mu, s, with_kappa=True):
    """Normwise scales of the two stresses.

    Corotated: 2 mu |F| (|F| + 1) + |lambda| (|J| + dJ) (|J| + 1), times s_max / s_kept_min unless `with_kappa` is False (the
    kernel forms (F - U V^T) F^T, and U's smallest kept column carries ~u s_max / s in direction; the trace of tau does
    not: tr(U (S - I) V^T F^T) = sum (s_i - 1) u_i . F v_i with u_i = F v_i / s_i).

    Neo-Hookean: mu |F|^2 + mu + |lambda| (|log J| + |F|^d / J) with J = max(det F, 1e-10) where the clamp may or may not
    act in fp32 (det's absolute round-off is ~u |F|^d, log divides it by J). Where det F lies below 1e-10 by more than
    that round-off the clamp has decided: log J = log 1e-10 whatever the rounding of det, and the scale is
    mu |F|^2 + mu + |lambda| |log 1e-10| — so the clamped pressure of an inverted element is held to u, not to 1e11 u."""
    d = F.shape[1]
    fn = np.linalg.norm(F, axis=(1, 2))
    if model == 0:
        J = np.prod(s, 1)
        abs_s = np.sort(np.abs(s), 1)[:, ::-1]
        # J = s_1 ... s_d carries the absolute error of its smallest factor (~u s_max) times the others: relative to |J| it
        # is unbounded as s_min -> 0, so the lambda term is scaled by |J| + s_max * (product of the d - 1 largest)
        jerr = abs_s[:, 0] * np.prod(abs_s[:, :-1], 1)
        base = 2.0 * np.abs(mu) * fn * (fn + 1.0) + np.abs(lam) * (np.abs(J) + jerr) * (np.abs(J) + 1.0)
        return base * kappa_kept(abs_s) if with_kappa else base
    det = np.linalg.det(F)
    clamped = det < NH_CLAMP - C_DEC * U32 * fn ** d
    j = np.maximum(det, NH_CLAMP)
    free = np.abs(mu) * fn * fn + np.abs(mu) + np.abs(lam) * (np.abs(np.log(j)) + fn ** d / j)
    decided = np.abs(mu) * fn * fn + np.abs(mu) + np.abs(lam) * abs(np.log(NH_CLAMP))
    return np.where(clamped, decided, free)


def check_tau(tag, model, tau, F, lam, mu, svd64, c=C_TAU):
    """Per-matrix checks of a device stress tau [n,d,d] against the fp64 truth of the same fp32 F [n,d,d] (float64 values).
    Returns the list of failures; every bound is reported.
    - normwise, C u scale (tau_scales); for corotated tau only where it is unique (tau_unique) — it carries the factor
      s_max / s_kept_min, so above kappa ~1e5 it no longer constrains tau and the trace check below carries the matrix;
    - corotated also the trace, every matrix: tr tau = 2 mu (|F|^2 - sum s) + d lambda (J - 1) J depends on the singular
      values only, bound C u d * scale without kappa."""
    d = F.shape[1]
    U, s, V = svd64
    t64 = tau_corotated64(F, lam, mu, U, s) if model == 0 else tau_neo_hookean64(F, lam, mu)
    fails = []

    def bound(name, err, b, sel):
        err, b = err[sel], np.maximum(b[sel], 1e-300)
        if not err.size:
            return
        w = int(np.argmax(err / b))
        report_margin(f"{tag}: {name}", float(err[w]), float(b[w]), n=int(err.size))
        bad = ~(err <= b)
        if bad.any():
            i = int(np.nonzero(sel)[0][np.argmax(bad)])
            fails.append(f"{tag}: {name}: {int(bad.sum())}/{err.size} over the bound (first #{i}: {err[np.argmax(bad)]:.3e} > "
                         f"{b[np.argmax(bad)]:.3e}; F = {F[i].tolist()}, lambda {lam[i]}, mu {mu[i]})")

    uniq = tau_unique(s) if model == 0 else np.ones(len(F), bool)
    bound("tau normwise", np.linalg.norm(tau - t64, axis=(1, 2)), c * U32 * tau_scales(model, F, lam, mu, s), uniq)
    if model == 0:
        terr = np.abs(np.trace(tau, axis1=1, axis2=2) - np.trace(t64, axis1=1, axis2=2))
        bound("tau trace (no kappa)", terr, c * U32 * d * tau_scales(model, F, lam, mu, s, with_kappa=False), np.ones(len(F), bool))
    return fails


def tau_unique(s):
    """corotated tau is unique unless det F < 0 with a tied smallest |s|, or two singular values vanish (rank <= d-2):
    U S U^T then depends on the choice of basis inside the tied subspace"""
    a, smax, gaps = sv_stats(s)
    tie = C_SV * U32 * smax * 4.0
    tied_small = np.abs(a[:, -1] - a[:, -2]) <= tie
    inverted = s.min(1) < -tie
    two_zero = a[:, -2] <= tie if s.shape[1] == 3 else np.zeros(len(s), bool)
    return ~((inverted & tied_small) | two_zero)


# ------------------------------------------------------------------------------------------------ truth: Drucker-Prager
def dp_alpha64(dp, q):
    angle = dp[:, 0] + (dp[:, 1] * q - dp[:, 3]) * np.exp(-dp[:, 2] * q)
    sa = np.sin(angle)
    return np.sqrt(2.0 / 3.0) * (2.0 * sa) / (3.0 - sa)


def dp_outcomes64(dp, state, F, svd, f_err=None):
    # F: [n, d, d] float64 (the fp32 input, unchanged by branch 'N')
    """fp64 Drucker-Prager (models/drucker_prager.wgsl) from an fp64 SVD, every branch evaluated: returns a dict with the
    decision quantities, the branch fp64 takes ('A' = projection to the tip, 'B' = onto the cone, 'N' = unchanged), the
    outcome (F', state') of each branch, and the fp32 band around each threshold.

    `f_err` [n] (None: 0, the input is an exact fp32 matrix): F is known only to within |dF|_F <= f_err — the matrix a kernel
    projects is its own fp32 F_trial = F + (grad dt) F, the truth holds the fp64 one (tests/plastic_truth.py passes
    transfer_truth's b_F). What that does to the bands and to the outcomes, to first order in f_err:

    singular values: |ds_i| <= |dF|_2 <= f_err (Weyl), and |ds|_2 <= |dF|_F (Mirsky). With f_err <= s_min / 2 every value on
    the segment between the two matrices is at least s_i - f_err >= s_i / 2, so a log-strain moves by at most
    f_err / (s_i - f_err) <= 2 f_err / s_i (this sum is added to band_strain: the trace moves by at most the sum, |dev| by
    at most the 2-norm of the movements, which is below it), and the whole strain vector by |d eps|_2 <= de := f_err /
    (s_min - f_err). gamma = |dev| + c tr (c = coef alpha) moves by at most (1 + |c|) times the strains' sum: the existing
    expression of band_gamma with the widened band_strain. A matrix with f_err > s_min / 2 may lose a singular value
    altogether: `amb_input`, every branch allowed, counted as decision-ambiguous.

    outcomes: each branch is an isotropic map F = U diag(s) V^T -> U diag(p(s)) V^T with p symmetric in s. In the frame of
    U, V and with E = U^T dF V its derivative is, entry by entry (Daleckii-Krein for singular values),
        diagonal       dp_i = sum_j (dp_i / ds_j) E_jj
        i != j         (p_i - p_j) / (s_i - s_j) * (E_ij + E_ji) / 2  +  (p_i + p_j) / (s_i + s_j) * (E_ij - E_ji) / 2,
    so |dF'|_F <= K |dF|_F with K the largest of the three kinds of coefficient.
      N: p = s, K = 1; the state does not move.
      A: p = 1: only the third kind is left, K = 2 / (s_i + s_j) at the two smallest values (the polar factor's bound).
         state: hard = |eps| moves by at most de; log prev_det by at most sqrt(d) de (Cauchy-Schwarz on the sum), and st0
         by |st0'| times that.
      B: p_i = exp(H_i), H = (tr / d) 1 - c tr nhat, nhat = dev / |dev|. |d tr| <= sqrt(d) |d eps|, |d nhat| <= |d eps| / |dev|,
         so |dH| <= (1 + sqrt(d) |c| + |c tr| / |dev|) |d eps| =: L |d eps| and the diagonal kind is at most p_max L / s_min.
         H_i - H_j = -(c tr / |dev|) (log s_i - log s_j), so the first kind is at most p_max |c tr| / (|dev| s_min), below
         it; the third is at most p_max / s_min, below it as well. K = p_max L / s_min — the cone map with the SVD's
         kappa (1 / s_min against p_max) and the 1 / |dev| of the direction. state: hard = gamma moves by at most
         (1 + sqrt(d) |c|) de, the two log dets by sqrt(d) de each.
    s_min, |dev|, |tr| and p_max are taken at their worst on the segment (s - f_err, |dev| - de, |tr| + sqrt(d) de, p_max
    exp(L de); the first two no further than a factor 2 from their value: beyond that the particle is ambiguous anyway).
    tests/test_plastic_truth.py draws dF at |dF|_F = f_err and holds every branch's movement below K f_err (`lip_F`,
    `lip_state` of each outcome)."""
    U, s, V = svd
    n, d = s.shape
    fe = np.zeros(n) if f_err is None else np.broadcast_to(np.asarray(f_err, np.float64), (n,))
    dp = np.asarray(dp, np.float64)
    state = np.asarray(state, np.float64)
    with np.errstate(all="ignore"):
        alpha = dp_alpha64(dp, state[:, 1])
        strain = np.log(s) + (state[:, 2] / d)[:, None]
        tr = strain.sum(1)
        dev = strain - (tr / d)[:, None]
        dev_norm = np.linalg.norm(dev, axis=1)
        coef = (d * dp[:, 4] + 2.0 * dp[:, 5]) / (2.0 * dp[:, 5])
        gamma = dev_norm + coef * tr * alpha
        a = np.abs(s)
        kap = a.max(1)[:, None] / a
        # fp32 band of the strains: logf of a singular value that carries ~u s_max of round-off, plus the log's own ulp
        band_fp32 = C_DEC * U32 * ((np.abs(np.log(a)) + kap).sum(1) + np.abs(state[:, 2]))
        band_strain = band_fp32 + (2.0 * fe[:, None] / a).sum(1)
        band_gamma = band_strain * (1.0 + np.abs(coef * alpha)) + C_DEC * U32 * (dev_norm + np.abs(coef * tr * alpha))
        amb_input = fe > 0.5 * a.min(1)
        # the segment's worst s, |dev|, |tr| (see the docstring); all of it exactly neutral at f_err = 0
        a_eff = np.maximum(a - fe[:, None], 0.5 * a)
        exact = fe == 0.0
        de = np.where(exact, 0.0, fe / a_eff.min(1))
        two = np.sort(a_eff, 1)[:, :2].sum(1)
        c_abs = np.abs(coef * alpha)
        dn_eff = np.maximum(dev_norm - de, 0.5 * dev_norm)
        lip_H = 1.0 + np.sqrt(d) * c_abs + c_abs * (np.abs(tr) + np.sqrt(d) * de) / np.maximum(dn_eff, 1e-300)
        all_zero = np.all(dev == 0.0, axis=1)
        branch = np.where((tr > 0) | all_zero, "A", np.where(gamma > 0, "B", "N"))
        amb_trace = np.abs(tr) <= band_strain
        amb_zero = (dev_norm <= band_strain) & ~(tr > band_strain)     # (a clear trace > 0 projects to the tip either way)
        amb_gamma = (np.abs(gamma) <= band_gamma) & (~(tr > 0) | amb_trace)   # (fp32 may land on the cone side of trace = 0)
        out = {}
        prev_det = np.prod(s, 1)
        for br in ("A", "B"):
            if br == "A":
                nsv = np.ones_like(s)
                hard = np.linalg.norm(strain, axis=1)
            else:
                nsv = np.exp(strain - dev * (gamma / dev_norm)[:, None])
                hard = gamma
            new_det = np.prod(nsv, 1)
            st = state.copy()
            st[:, 0] = state[:, 0] * prev_det / new_det
            st[:, 2] = state[:, 2] + np.log(prev_det) - np.log(new_det)
            st[:, 1] = state[:, 1] + hard
            Fn = (U * nsv[:, None, :]) @ np.transpose(V, (0, 2, 1))
            # normwise scales of the outputs: U's direction error (kappa) and the logs / exps of the strains; on the cone
            # also the direction dev / |dev|, which carries the strains' band over |dev|
            rel = kap.max(1) + np.abs(strain).sum(1) + 1.0
            if br == "B":
                rel = rel + np.abs(gamma) * band_fp32 / (C_DEC * U32) / np.maximum(dev_norm, 1e-300)
            if br == "A":
                lip_F = np.where(exact, 0.0, 2.0 * fe / two)
                lip_state = np.stack([np.abs(st[:, 0]) * np.sqrt(d) * de, de, np.sqrt(d) * de], 1)
            else:
                lip_F = np.where(exact, 0.0, nsv.max(1) * np.exp(lip_H * de) * lip_H * de)
                lip_state = np.stack([np.abs(st[:, 0]) * 2.0 * np.sqrt(d) * de, (1.0 + np.sqrt(d) * c_abs) * de, 2.0 * np.sqrt(d) * de], 1)
            lip_state = np.where(exact[:, None], 0.0, lip_state)
            out[br] = dict(F=Fn, state=st, rel=rel, hard=hard, new_det=new_det, lip_F=lip_F, lip_state=lip_state)
        out["N"] = dict(F=np.asarray(F, np.float64), state=state.copy(), rel=np.ones(n),
                        hard=np.zeros(n), new_det=prev_det, lip_F=fe, lip_state=np.zeros((n, 3)))
    return dict(branch=branch, tr=tr, gamma=gamma, dev_norm=dev_norm, amb_trace=amb_trace, amb_zero=amb_zero,
                amb_gamma=amb_gamma, amb_input=amb_input, out=out, prev_det=prev_det)


def dp_allowed(res):
    """[n] list of the branches a correct fp32 evaluation may take: the fp64 one, and across every threshold the fp64
    values put within the fp32 band, the branch on its other side (computed once per `res`: dp_match asks per particle)"""
    if "_allowed" in res:
        return res["_allowed"]
    allowed = res["_allowed"] = []
    for i, br in enumerate(res["branch"]):
        s = {br}
        other = "B" if res["gamma"][i] > 0 else "N"
        if res["amb_trace"][i] or res["amb_zero"][i]:
            s |= {"A", other}
        if res["amb_gamma"][i]:
            s |= {"B", "N"}
        if res["amb_input"][i]:
            s = {"A", "B", "N"}
        allowed.append(s)
    return allowed


def dp_match(res, i, changed, F_gpu, st_gpu, fnorm_in):
    """(branch it matches or None, worst measured / bound over F', state). F_gpu [d,d], st_gpu [3]."""
    best = (None, np.inf)
    for br in dp_allowed(res)[i]:
        o = res["out"][br]
        if bool(changed) != (br != "N"):
            continue
        Fo, so = o["F"][i], o["state"][i]
        scale_F = max(np.linalg.norm(Fo), fnorm_in) * o["rel"][i]
        lf, ls = o["lip_F"][i], o["lip_state"][i]      # (the input's own uncertainty, dp_outcomes64: 0.0 for an exact input)
        r = [np.linalg.norm(F_gpu - Fo) / (C_DP * U32 * scale_F + lf)]
        if br != "N":
            prev, new = abs(res["prev_det"][i]), abs(o["new_det"][i])
            r.append(abs(st_gpu[0] - so[0]) / (C_DP * U32 * abs(so[0]) * o["rel"][i] * 4.0 + 1e-300 + ls[0]))
            r.append(abs(st_gpu[1] - so[1]) / (C_DP * U32 * (abs(so[1]) + o["rel"][i] * (abs(o["hard"][i]) + 1.0)) + 1e-300 + ls[1]))
            r.append(abs(st_gpu[2] - so[2]) / (C_DP * U32 * (abs(so[2]) + abs(np.log(prev)) + abs(np.log(new)) + o["rel"][i]) + 1e-300 + ls[2]))
        else:
            r.append(float(np.max(np.abs(st_gpu - so))) / (C_DP * U32 * (np.abs(so).max() + 1.0)))
        w = float(max(r))
        if w < best[1]:
            best = (br, w)
    return best
