"""-m "not gpu": tests/emit_truth.py checked against itself — the mixer against hand-computed vectors and a second statement, the
jitter's range, the lattice's box, the schedule against its closed form, the capacity rule."""
import numpy as np
import pytest

import emit_truth as ET
from wgsparkl_amd import _ffi
from wgsparkl_amd.models import ElasticCoefficients, Emitter
from wgsparkl_amd.solver import ParticleSet

# computed by hand from the header's five lines (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16)
VECTORS = {0x0: 0x0, 0x1: 0x688990c0, 0x2: 0xd1132181, 0x9e3779b9: 0x01fce552, 0xffffffff: 0x6768824a, 0x3039: 0x912efcf7}


def proto(dim, vel=None):
    ps = ParticleSet.uniform(np.zeros((1, dim), np.float32), 0.25, 1000.0, ElasticCoefficients.from_young_modulus(1e5, 0.3))
    if vel is not None:
        ps.vel[0] = vel
    return ps


def emitter(dim, **kw):
    args = dict(lo=(1.0, 2.0, 3.0)[:dim], count=(3, 4, 2)[:dim], spacing=0.5, jitter=0.25, seed=77)
    args.update(kw)
    return Emitter(proto(dim), **args)


def test_the_mixer_against_hand_computed_vectors_and_every_other_statement_of_it():
    for x, want in VECTORS.items():
        assert ET.lowbias32_int(x) == want
        assert int(ET.lowbias32(np.array([x], np.uint32))[0]) == want
        assert int(_ffi.lowbias32(np.array([x], np.uint32))[0]) == want
    xs = np.random.default_rng(3).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ET.lowbias32(xs), np.array([ET.lowbias32_int(int(x)) for x in xs], np.uint32))
    assert len(np.unique(ET.lowbias32(np.arange(1 << 16, dtype=np.uint32)))) == 1 << 16     # (a bijection: no two inputs collide)


@pytest.mark.parametrize("dim", [2, 3])
def test_every_u_lies_in_the_half_open_interval_and_depends_on_all_five_inputs(dim):
    u = ET.jitter_u(123, 2, 5, 50000, dim)
    assert u.dtype == np.float32 and u.shape == (50000, dim)
    assert u.min() >= -0.5 and u.max() < 0.5
    assert abs(float(u.mean())) < 0.01 and 0.27 < float(u.std()) < 0.30           # uniform: std = 1 / sqrt(12)
    for other in (ET.jitter_u(124, 2, 5, 50000, dim), ET.jitter_u(123, 3, 5, 50000, dim), ET.jitter_u(123, 2, 6, 50000, dim)):
        assert (other != u).mean() > 0.99
    assert np.array_equal(ET.jitter_u(123, 2, 5, 100, dim), u[:100])             # a point's value does not depend on the batch's size
    # the extreme hashes: 0 -> -0.5 exactly, 0xffffffff -> 0.5 - 2^-24 exactly
    assert np.float32(0) * np.float32(2.0 ** -24) - np.float32(0.5) == -0.5
    assert np.float32(0xffffff) * np.float32(2.0 ** -24) - np.float32(0.5) == np.float32(0.5 - 2.0 ** -24) < 0.5


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("jitter", [0.0, 0.25, 0.5])
def test_every_point_lies_in_the_lattice_box_widened_by_the_jitter(dim, jitter):
    em = emitter(dim, jitter=jitter, count=(5, 3, 4)[:dim], lo=(-3.7, 0.1, 12.3)[:dim], spacing=0.37)
    x = ET.batch_positions(em, 1, 9).astype(np.float64)
    assert x.shape == (em.batch_size, dim)
    lo = np.asarray(em.lo, np.float64)
    hi = lo + np.asarray(em.count) * 0.37
    slack = jitter * 0.37 * 0.5 + 1e-5
    assert (x >= lo - slack).all() and (x <= hi + slack).all()
    idx = ET.lattice_indices(em.count)
    assert np.array_equal(idx[1], [1] + [0] * (dim - 1)) and np.array_equal(idx[5], [0, 1] + [0] * (dim - 2))       # x fastest
    centre = lo + (idx + 0.5) * 0.37
    assert np.abs(x - centre).max() <= slack
    if jitter == 0.0:
        cell = idx.astype(np.float32) + np.float32(0.5)
        assert np.array_equal(ET.batch_positions(em, 1, 9), np.asarray(em.lo, np.float32) + cell * np.float32(0.37))
    elif jitter == 0.5:
        assert np.abs(x - centre).max() > 0.8 * (0.5 * 0.37 * 0.5)                   # the jitter is used to its width: |u| up to 1/2


def test_the_batch_count_over_a_run_equals_the_closed_form():
    for start, period, batches in ((0, 1, 0), (0, 3, 0), (5, 4, 0), (2, 7, 3), (30, 2, 0), (0, 5, 1), (11, 1, 4)):
        em = emitter(2, start_substep=start, period=period, batches=batches)
        for substeps in (0, 1, 5, 11, 12, 29, 30, 31, 64):
            fired = [ET.due(em, s) for s in range(substeps)]
            got = [q for q in fired if q is not None]
            assert got == list(range(len(got))), "the batch numbers count up from 0"
            assert len(got) == ET.scheduled_batches(em, substeps), (start, period, batches, substeps)
            events, emitted, skipped, n = ET.run_schedule([em], 10, 10 ** 9, substeps)
            assert len(events) == len(got) and emitted == [len(got) * em.batch_size] and skipped == [0] and n == 10 + emitted[0]
    # a run in pieces is the run in one piece
    ems = [emitter(2, start_substep=1, period=3), emitter(2, start_substep=0, period=5, count=(2, 2))]
    whole = ET.run_schedule(ems, 0, 10 ** 9, 24)
    ev, n = [], 0
    for first, k in ((0, 1), (1, 5), (6, 18)):
        part = ET.run_schedule(ems, n, 10 ** 9, k, first)
        ev, n = ev + part[0], part[3]
    assert ev == whole[0] and n == whole[3]
    assert whole[0][:2] == [(0, 1, 0), (1, 0, 0)]              # substep 0: emitter 1 alone; substep 1: emitter 0
    assert [(e, q) for s, e, q in whole[0] if s == 10] == [(0, 3), (1, 2)]         # both due: array order


def test_a_batch_that_does_not_fit_is_skipped_whole_and_a_later_one_is_tried_again():
    big = emitter(2, count=(4, 3), period=2)                  # 12 per batch, substeps 0, 2, 4, ..
    small = emitter(2, count=(2, 1), period=3)                # 2 per batch, substeps 0, 3, 6, ..
    events, emitted, skipped, n = ET.run_schedule([big, small], 0, 30, 8)
    # 0: +12 +2 = 14 | 2: +12 = 26 | 3: +2 = 28 | 4: 12 does not fit | 6: 12 does not fit, +2 = 30
    assert events == [(0, 0, 0), (0, 1, 0), (2, 0, 1), (3, 1, 1), (6, 1, 2)]
    assert emitted == [24, 6] and skipped == [2, 0] and n == 30
    # the skipped batch numbers are not made up for: batch 2 and 3 of `big` never come
    assert [q for _, e, q in events if e == 0] == [0, 1]
    # room again (a larger capacity from the start): the same emitter's later batches fit
    assert ET.run_schedule([big, small], 0, 64, 8)[2] == [0, 0]


def test_a_batch_of_particles_is_the_proto_at_the_lattice():
    em = Emitter(proto(3, vel=(0.0, -2.0, 0.5)), (0.0, 5.0, 0.0), (2, 2, 2), 0.5, jitter=0.1, seed=4)
    ps = ET.batch_particles(em, 0, 3)
    assert ps.n == 8 and np.array_equal(ps.pos, ET.batch_positions(em, 0, 3))
    assert np.array_equal(ps.vel, np.tile(np.float32([0.0, -2.0, 0.5]), (8, 1))) and np.array_equal(ps.mass, np.repeat(em.proto.mass, 8))
    assert em.proto.n == 1                                     # (the proto is not touched)
