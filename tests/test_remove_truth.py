"""-m "not gpu": tests/remove_truth.py held to the properties include/wgsparkl_hip_remove.h states — the truth the GPU tests remove by
must itself be right: a particle on a face is inside, a NaN is inside nothing and an OUTSIDE sink takes it, INSIDE and OUTSIDE partition
every particle set, kept_from is increasing and inverts new_index, the schedule's closed form, the first-sink attribution."""
import collections

import numpy as np
import pytest

import remove_truth as RT

F32 = np.float32
Sink = collections.namedtuple("Sink", "region side center half start_substep period", defaults=(0, 1))


def box(center, half, side=RT.SINK_INSIDE, **kw):
    return Sink(RT.REGION_BOX, side, tuple(center), tuple(half), **kw)


def ball(center, radius, side=RT.SINK_INSIDE, **kw):
    return Sink(RT.REGION_BALL, side, tuple(center), (radius, 0.0, 0.0), **kw)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_particle_on_a_face_is_inside(dim):
    c, half = (4.0, 2.0, 8.0), (1.5, 0.25, 3.0)          # exactly representable: the faces are, too
    b = box(c, half)
    for k in range(dim):
        for sign in (-1.0, 1.0):
            on = np.array([c[:dim]], F32)
            on[0, k] = c[k] + sign * half[k]
            beyond = on.copy()
            beyond[0, k] = np.nextafter(on[0, k], F32(sign * np.inf), dtype=F32)
            assert RT.inside(b, on)[0] and not RT.inside(b, beyond)[0], (k, sign)
    # the third components are ignored in 2D
    if dim == 2:
        assert RT.inside(box((4.0, 2.0, 1e9), (1.5, 0.25, 0.0)), np.array([[4.0, 2.0]], F32))[0]
    r = ball(c, 2.5)
    on = np.array([c[:dim]], F32)
    on[0, 0] += 2.5
    assert RT.inside(r, on)[0]
    on[0, 0] = np.nextafter(on[0, 0], F32(np.inf), dtype=F32)
    assert not RT.inside(r, on)[0]
    # the ball's sum in fp32, term by term: 3-4-5 scaled is exact
    p = np.array([[c[0] + 1.5, c[1] + 2.0, c[2]][:dim]], F32)
    assert RT.inside(ball(c, 2.5), p)[0] and not RT.inside(ball(c, np.nextafter(F32(2.5), F32(0.0))), p)[0]


@pytest.mark.parametrize("dim", [2, 3])
def test_a_nan_is_inside_nothing_and_outside_takes_it(dim):
    pos = np.zeros((dim + 1, dim), F32)
    for k in range(dim):
        pos[k, k] = np.nan
    pos[dim, 0] = np.inf
    for make in (lambda side: box((0.0, 0.0, 0.0), (1e30, 1e30, 1e30), side), lambda side: ball((0.0, 0.0, 0.0), 1e18, side)):
        assert not RT.inside(make(RT.SINK_INSIDE), pos).any()
        assert not RT.takes(make(RT.SINK_INSIDE), pos).any() and RT.takes(make(RT.SINK_OUTSIDE), pos).all()


@pytest.mark.parametrize("dim", [2, 3])
def test_inside_and_outside_partition_every_particle_set(dim):
    rng = np.random.default_rng(3 + dim)
    pos = rng.uniform(-4.0, 4.0, (4000, dim)).astype(F32)
    pos[::97] = np.nan
    pos[::89, 0] = F32(1.5)                                  # some on a face
    for region in (box((0.5, -0.25, 0.0), (1.0, 2.0, 3.0)), ball((0.5, -0.25, 0.0), 2.0)):
        a, b = RT.takes(region, pos), RT.takes(region._replace(side=RT.SINK_OUTSIDE), pos)
        assert (a ^ b).all() and a.any() and b.any()
    # fp32, not fp64: x - c = 2 + 1e-8 is outside a half of 2 in exact arithmetic; fl(x - c) is 2, on the face
    assert RT.inside(box((-1e-8, 0.0, 0.0), (2.0, 1.0, 1.0)), np.array([[2.0] + [0.0] * (dim - 1)], F32))[0]


def test_renumbering_and_kept_from():
    rng = np.random.default_rng(11)
    for n in (0, 1, 64, 1000):
        for p in (0.0, 0.3, 1.0):
            remove = (rng.uniform(size=n) < p).astype(np.uint8) * 7      # nonzero means remove
            new_index, kept_from = RT.renumber(remove)
            assert kept_from.size == int((remove == 0).sum()) and (np.diff(kept_from.astype(np.int64)) > 0).all()
            assert np.array_equal(new_index[kept_from], np.arange(kept_from.size))
            # the new index is the old index minus the removed particles in front of it
            removed_before = np.cumsum(remove != 0) - (remove != 0)
            assert np.array_equal(new_index[kept_from], kept_from - removed_before[kept_from])
    new_index, kept_from = RT.renumber([0, 1, 1, 0, 0, 1, 0])
    assert list(kept_from) == [0, 3, 4, 6] and list(new_index) == [0, 1, 1, 1, 2, 3, 3]


def test_schedule_and_attribution():
    a, b = box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), start_substep=2, period=3), ball((0.0, 0.0, 0.0), 2.0, start_substep=0, period=4)
    assert [s for s in range(12) if RT.due(a, s)] == [2, 5, 8, 11] and [s for s in range(12) if RT.due(b, s)] == [0, 4, 8]
    assert RT.due_sinks([a, b], 8) == [0, 1] and RT.due_sinks([a, b], 3) == [] and RT.due_sinks([a, b], 4) == [1]
    for k in (a, b, box((0.0,) * 3, (1.0,) * 3, start_substep=7, period=1)):
        for n in range(0, 30):
            assert RT.firings(k, n) == sum(RT.due(k, s) for s in range(n)), (k, n)
    pos = np.array([[0.5, 0.5, 0.5], [1.5, 0.0, 0.0], [3.0, 0.0, 0.0]], F32)
    remove, taker = RT.attribute([a, b], pos)
    assert list(remove) == [True, True, False] and list(taker) == [0, 1, -1] and RT.counts([a, b], pos) == [1, 1]
    assert RT.counts([b, a], pos) == [2, 0]                 # a particle in several counts for the first
    out = a._replace(side=RT.SINK_OUTSIDE)
    assert RT.counts([a, out], pos) == [1, 2] and RT.attribute([a, out], pos)[0].all()
