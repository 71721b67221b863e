"""fp64 / exact-integer truth for the device-side diagnostics (include/wgsparkl_hip.h "Device-side diagnostics"): the terms of every
sum in numpy float64, the fixed-point sums as Python integers, the bounds, and the digest. Independent of the HIP code: it follows
the definitions of the header, nothing else. Takes ParticleSets (wgs_read_particles order and conventions: matrices column-major)."""
import numpy as np

from oracle.np_oracle import mat64 as _mat

MODEL_COROTATED, MODEL_NEO_HOOKEAN = 0, 1
SUM_COMPONENTS_3D = dict(mass=1, momentum=3, angular=3, mass_moment=3, kinetic=1, kinetic_affine=1, elastic=1, gravity_potential=1)
U64 = np.uint64
GOLDEN, SECOND = U64(0x9e3779b97f4a7c15), U64(0xd1b54a32d192ed03)


# ---------------------------------------------------------------------------------------------- elastic energy
def psi_parts(model, F, lam, mu):
    """The additive pieces of Psi(F) (F: [n, d, d], lam / mu: [n]) -> [n, pieces]. Corotated (linear_elasticity.wgsl:28-41):
    mu * sum (s_i - 1)^2, lambda/2 (J - 1)^2; neo-Hookean (neo_hookean_elasticity.wgsl:14-25): mu/2 (tr F^T F - d), -mu ln J,
    lambda/2 ln^2 J with J = max(det F, 1e-10). Evaluated through G = F - I so that nothing cancels near the rest state."""
    F = np.asarray(F, np.float64)
    n, d, _ = F.shape
    lam, mu = np.broadcast_to(np.asarray(lam, np.float64), (n,)), np.broadcast_to(np.asarray(mu, np.float64), (n,))
    G = F - np.eye(d)
    E = G + G.transpose(0, 2, 1) + G.transpose(0, 2, 1) @ G          # F^T F - I
    tr = np.trace(G, axis1=1, axis2=2)
    if d == 2:
        jm1 = tr + np.linalg.det(G)
    else:
        i2 = 0.5 * (tr * tr - np.trace(G @ G, axis1=1, axis2=2))
        jm1 = tr + i2 + np.linalg.det(G)
    if model == MODEL_NEO_HOOKEAN:
        lnj = np.where(1.0 + jm1 >= 1.0e-10, np.log1p(np.maximum(jm1, -1.0 + 1.0e-10)), np.log(1.0e-10))
        return np.stack([0.5 * mu * np.trace(E, axis1=1, axis2=2), -mu * lnj, 0.5 * lam * lnj * lnj], 1)
    ev = np.linalg.eigvalsh(E)                                          # ascending
    s = np.sqrt(np.maximum(1.0 + ev, 0.0))
    sm1 = ev / (s + 1.0)                                                # s - 1
    flipped = 1.0 + jm1 < 0.0                                           # det F < 0: the smallest singular value carries the sign
    sm1[flipped, 0] = -(s[flipped, 0] + 1.0)
    return np.stack([mu * np.sum(sm1 * sm1, 1), 0.5 * lam * jm1 * jm1], 1)


def psi(model, F, lam=1.0, mu=1.0):
    F = np.asarray(F, np.float64)
    single = F.ndim == 2
    out = psi_parts(model, F[None] if single else F, lam, mu).sum(1)
    return float(out[0]) if single else out


# ---------------------------------------------------------------------------------------------- sums
def finite_mask(ps):
    cols = [ps.pos, ps.vel, ps.def_grad, ps.affine, ps.mass[:, None], ps.init_volume[:, None], ps.lambda_[:, None], ps.mu[:, None]]
    return np.all(np.isfinite(np.concatenate([np.asarray(c, np.float64) for c in cols], 1)), 1)


def terms(ps, h, gravity, model=MODEL_COROTATED, energy=True):
    """name -> [n_finite, components] float64 terms of the particle sums, and name -> [n_finite] sums of the absolute values of the
    pieces a term is added up from (what a forward error bound of its fp64 evaluation is relative to)."""
    d = ps.dim
    keep = finite_mask(ps)
    f = lambda a: np.asarray(a, np.float64)[keep]
    m, x, v, A = f(ps.mass), f(ps.pos), f(ps.vel), _mat(f(ps.affine), d)
    g = np.asarray(list(gravity), np.float32).astype(np.float64)[:d]      # (wgs_sim_params is fp32)
    h2q = 0.25 * float(np.float32(h)) ** 2
    t, mag = {}, {}
    t["mass"] = m[:, None]
    t["momentum"] = m[:, None] * v
    t["mass_moment"] = m[:, None] * x
    if d == 3:
        orb = m[:, None] * np.cross(x, v)
        ax = np.stack([A[:, 2, 1] - A[:, 1, 2], A[:, 0, 2] - A[:, 2, 0], A[:, 1, 0] - A[:, 0, 1]], 1)
        mag["angular"] = (np.abs(m)[:, None] * (np.abs(x[:, [1, 2, 0]] * v[:, [2, 0, 1]]) + np.abs(x[:, [2, 0, 1]] * v[:, [1, 2, 0]])) +
                          h2q * np.stack([np.abs(A[:, 2, 1]) + np.abs(A[:, 1, 2]), np.abs(A[:, 0, 2]) + np.abs(A[:, 2, 0]),
                                          np.abs(A[:, 1, 0]) + np.abs(A[:, 0, 1])], 1))
    else:
        orb = (m * (x[:, 0] * v[:, 1] - x[:, 1] * v[:, 0]))[:, None]
        ax = (A[:, 1, 0] - A[:, 0, 1])[:, None]
        mag["angular"] = (np.abs(m) * (np.abs(x[:, 0] * v[:, 1]) + np.abs(x[:, 1] * v[:, 0])) + h2q * (np.abs(A[:, 1, 0]) + np.abs(A[:, 0, 1])))[:, None]
    t["angular"] = orb + h2q * ax
    t["kinetic"] = (0.5 * m * np.sum(v * v, 1))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t["kinetic_affine"] = np.where(m != 0.0, 0.5 * h2q * np.sum(A * A, (1, 2)) / m, 0.0)[:, None]
    t["gravity_potential"] = (-(m * (x @ g)))[:, None]
    mag["gravity_potential"] = (np.abs(m) * (np.abs(x) @ np.abs(g)))[:, None]
    if energy:
        parts = f(ps.init_volume)[:, None] * psi_parts(model, _mat(f(ps.def_grad), d), f(ps.lambda_), f(ps.mu))
        t["elastic"] = parts.sum(1)[:, None]
        mag["elastic"] = np.abs(parts).sum(1)[:, None]
    for k in t:
        mag.setdefault(k, np.abs(t[k]))
    return t, mag


def nbits(n):
    return int(n).bit_length()


def exponent_of(max_abs_term, count):
    """exponent = b + nbits(N) - 62 (header): b = frexp exponent of the largest |term|, -200 when it is zero."""
    b = int(np.frexp(float(max_abs_term))[1]) if max_abs_term > 0 else -200
    return max(-1000, min(1000, b + nbits(count) - 62))


def fixed_sum(term_column, exponent):
    """sum of rint(term * 2^-exponent) as a Python integer (exact)."""
    scaled = np.rint(np.ldexp(np.asarray(term_column, np.float64), -int(exponent)))
    return sum(int(s) for s in scaled)


def exact_sums(ps, h, gravity, model=MODEL_COROTATED, energy=True, count=None):
    """name -> (list of Python-integer fixed sums per component, exponent), as the header prescribes, from THIS module's terms."""
    t, _ = terms(ps, h, gravity, model, energy)
    n = ps.n if count is None else count
    out = {}
    for name, col in t.items():
        e = exponent_of(np.max(np.abs(col)) if col.size else 0.0, n)
        out[name] = ([fixed_sum(col[:, k], e) for k in range(col.shape[1])], e)
    return out


def bounds(ps, h, dt):
    """The bounds over the finite particles: exact ones in fp32, computed ones in fp64 (the caller rounds / allows ulps)."""
    d = ps.dim
    keep = finite_mask(ps)
    x, v = ps.pos[keep], ps.vel[keep]
    F, A = _mat(ps.def_grad[keep], d), np.asarray(ps.affine[keep], np.float64)
    m, vol, lam, mu = (np.asarray(a[keep], np.float64) for a in (ps.mass, ps.init_volume, ps.lambda_, ps.mu))
    vinf = np.float32(np.max(np.abs(v))) if len(v) else np.float32(0)
    w2 = np.where(m > 0, (lam + 2.0 * mu) * vol / np.where(m > 0, m, 1.0), 0.0)
    return dict(aabb_min=x.min(0), aabb_max=x.max(0), max_speed=np.sqrt(np.sum(np.asarray(v, np.float64) ** 2, 1)).max(),
                max_affine_norm=np.sqrt(np.sum(A * A, 1)).max(), det=np.linalg.det(F),
                max_wave_speed=np.sqrt(np.maximum(w2, 0.0)).max(), cfl=(vinf * np.float32(dt)) / np.float32(h))


def grid_terms(cells, vel_mass, h, dim):
    """Terms of the three grid sums from read_grid() records: m_i, m_i v_i, m_i (x_i cross v_i), x_i = cell * h; and the sums of the
    absolute values of the pieces they are added up from."""
    m = np.asarray(vel_mass[:, dim], np.float64)
    v = np.asarray(vel_mass[:, :dim], np.float64)
    x = np.asarray(cells, np.float64) * float(np.float32(h))
    ang = m[:, None] * np.cross(x, v) if dim == 3 else (m * (x[:, 0] * v[:, 1] - x[:, 1] * v[:, 0]))[:, None]
    if dim == 3:
        amag = np.abs(m)[:, None] * (np.abs(x[:, [1, 2, 0]] * v[:, [2, 0, 1]]) + np.abs(x[:, [2, 0, 1]] * v[:, [1, 2, 0]]))
    else:
        amag = (np.abs(m) * (np.abs(x[:, 0] * v[:, 1]) + np.abs(x[:, 1] * v[:, 0])))[:, None]
    t = dict(grid_mass=m[:, None], grid_momentum=m[:, None] * v, grid_angular=ang)
    return t, dict(grid_mass=np.abs(t["grid_mass"]), grid_momentum=np.abs(t["grid_momentum"]), grid_angular=amag)


# ---------------------------------------------------------------------------------------------- digest
def mix(z):
    z = np.asarray(z, U64)
    z = (z ^ (z >> U64(30))) * U64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> U64(27))) * U64(0x94d049bb133111eb)
    return z ^ (z >> U64(31))


def particle_hashes(ids, words):
    """ids [n] uint32, words [n, W] uint32 (x, v, F, A, plastic state, phase) -> H(p) [n] uint64 (header)."""
    with np.errstate(over="ignore"):
        w = np.asarray(words, np.uint32)
        if w.shape[1] % 2:
            w = np.concatenate([w, np.zeros((len(w), 1), np.uint32)], 1)
        h = mix(np.asarray(ids, np.uint32).astype(U64) + GOLDEN)
        for k in range(0, w.shape[1], 2):
            h = mix(h + GOLDEN + (w[:, k].astype(U64) | (w[:, k + 1].astype(U64) << U64(32))))
        return h


def words_of(ps, phase_words=True):
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(ps.n, -1)
    phase = u(ps.phase) if phase_words else np.zeros((ps.n, 2), np.uint32)
    return np.concatenate([u(ps.pos), u(ps.vel), u(ps.def_grad), u(ps.affine), u(ps.dp_state), phase], 1)


def digest_of_hashes(h):
    with np.errstate(over="ignore"):
        return (int(np.sum(h, dtype=U64)), int(np.sum(mix(h + SECOND), dtype=U64)))


def digest(ps, ids=None, phase_words=True):
    """(digest[0], digest[1]) of a ParticleSet as read back; ids default to the row index (the caller's order)."""
    ids = np.arange(ps.n, dtype=np.uint32) if ids is None else ids
    return digest_of_hashes(particle_hashes(ids, words_of(ps, phase_words)))
