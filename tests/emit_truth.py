"""The numpy restatement of include/wgsparkl_hip_emit.h's emitters: the integer mixer, the jitter, the lattice (every rounding an fp32
numpy operation of its own, as the header writes it) and the schedule with its capacity rule. Pure fp32 / uint32 arithmetic: what this
file computes is what the device writes, bit for bit — tests/test_gpu_emit.py appends these batches by hand and asks for the same bits.
Nothing here imports the library."""
import copy

import numpy as np

F32, U32 = np.float32, np.uint32


def lowbias32(x):
    """wgs_lowbias32 on uint32 arrays (arithmetic modulo 2^32)."""
    x = np.array(x, U32, ndmin=1)
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16))
        x = x * U32(0x7feb352d)
        x = x ^ (x >> U32(15))
        x = x * U32(0x846ca68b)
        x = x ^ (x >> U32(16))
    return x


def lowbias32_int(x):
    """the same on a Python integer, written with masks: the independent statement the hand-computed vectors are checked against"""
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def jitter_u(seed, e, q, npoints, dim):
    """u_k of every point of batch q of emitter e: [npoints, dim] float32 in [-0.5, 0.5)"""
    with np.errstate(over="ignore"):
        batch_hash = lowbias32(np.array([q], U32) * U32(0x9E3779B9) + U32(e))[0]
        idx = np.arange(npoints, dtype=U32)[:, None] * U32(dim) + np.arange(dim, dtype=U32)[None, :]
        h = lowbias32((U32(seed) ^ batch_hash ^ lowbias32(idx.reshape(-1))).reshape(-1)).reshape(npoints, dim)
    r = (h >> U32(8)).astype(F32)
    r01 = r * F32(2.0 ** -24)
    return r01 - F32(0.5)


def lattice_indices(count):
    """(i_0, ..) of every point, x fastest: [prod(count), dim] uint32"""
    count = [int(c) for c in count]
    t = np.arange(int(np.prod(count, dtype=np.int64)), dtype=np.int64)
    out = []
    for c in count:
        out.append(t % c)
        t = t // c
    return np.stack(out, 1).astype(U32)


def batch_positions(em, e, q):
    """x_k = fl(fl(lo_k + fl(fl((float)i_k + 0.5f) * spacing)) + fl(fl(jitter * spacing) * u_k)), [prod(count), dim] float32"""
    dim = len(em.count)
    idx = lattice_indices(em.count)
    u = jitter_u(em.seed, e, q, idx.shape[0], dim)
    spacing, jitter = F32(em.spacing), F32(em.jitter)
    cell = idx.astype(F32) + F32(0.5)
    off = cell * spacing
    at = np.asarray(em.lo, F32)[None, :] + off
    js = jitter * spacing
    jit = js * u
    return (at + jit).astype(F32)


def batch_particles(em, e, q):
    """the ParticleSet of batch q of emitter e: the proto, tiled, at the lattice's positions"""
    pos = batch_positions(em, e, q)
    ps = copy.copy(em.proto)
    for k, v in list(ps.__dict__.items()):
        if isinstance(v, np.ndarray):
            setattr(ps, k, np.repeat(v, pos.shape[0], axis=0))
    ps.pos = pos
    return ps


def due(em, s):
    """the batch number emitter `em` emits in front of the substep whose substeps_done value is s, or None"""
    if s < em.start_substep or (s - em.start_substep) % em.period != 0:
        return None
    q = (s - em.start_substep) // em.period
    return None if (em.batches != 0 and q >= em.batches) else q


def scheduled_batches(em, substeps):
    """closed form: the batches `em` has due in front of substeps 0 .. substeps - 1"""
    if substeps <= em.start_substep:
        return 0
    m = (substeps - 1 - em.start_substep) // em.period + 1
    return min(m, em.batches) if em.batches else m


def run_schedule(emitters, n0, capacity, substeps, first=0):
    """The schedule over substeps first .. first + substeps - 1 with the capacity rule: (events, emitted, skipped, n) — events = [(s, e, q)]
    of the batches that fit, in firing order; emitted = particles per emitter; skipped = batches per emitter that did not fit whole."""
    n = int(n0)
    events, emitted, skipped = [], [0] * len(emitters), [0] * len(emitters)
    for s in range(first, first + substeps):
        for e, em in enumerate(emitters):
            q = due(em, s)
            if q is None:
                continue
            size = int(np.prod([int(c) for c in em.count], dtype=np.int64))
            if n + size > capacity:
                skipped[e] += 1
                continue
            events.append((s, e, q))
            emitted[e] += size
            n += size
    return events, emitted, skipped, n
