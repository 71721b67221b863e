"""The numpy restatement of include/wgsparkl_hip_remove.h: the regions' membership (every rounding an fp32 numpy operation of its own, as
the header writes it), the first-sink attribution, the renumbering with kept_from, and the sinks' schedule. Pure fp32 / integer
arithmetic: what this file computes is what the device decides, bit for bit — tests/test_gpu_remove.py removes by these masks and asks for
the same survivors. Nothing here imports the library; a sink is anything with region, side, center, half, start_substep, period."""
import numpy as np

F32 = np.float32
REGION_BOX, REGION_BALL = 1, 2
SINK_INSIDE, SINK_OUTSIDE = 0, 1


def inside(sink, pos):
    """membership of every row of pos ([n, dim] float32) in the sink's REGION (its side not applied): bool [n]"""
    pos = np.asarray(pos, F32)
    dim = pos.shape[1]
    c, half = np.asarray(sink.center, F32), np.asarray(sink.half, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [pos[:, k] - c[k] for k in range(dim)]                      # d_k = fl(x_k - c_k)
        if int(sink.region) == REGION_BOX:
            out = np.ones(pos.shape[0], bool)
            for k in range(dim):
                out &= np.abs(d[k]) <= half[k]                           # a NaN compares false
            return out
        if int(sink.region) != REGION_BALL:
            raise ValueError("a sink's region is a box or a ball")
        s = d[0] * d[0]                                                  # s = fl(d_0 * d_0)
        for k in range(1, dim):
            t = d[k] * d[k]
            s = s + t                                                    # s = fl(s + fl(d_k * d_k))
        return s <= half[0] * half[0]


def takes(sink, pos):
    """the particles the sink removes: inside for SINK_INSIDE, NOT inside for SINK_OUTSIDE"""
    m = inside(sink, pos)
    return ~m if int(sink.side) == SINK_OUTSIDE else m


def attribute(sinks, pos):
    """(remove mask, taker): taker[i] = index of the first sink in array order that takes particle i, -1 if none does"""
    taker = np.full(np.asarray(pos).shape[0], -1, np.int64)
    for e in reversed(range(len(sinks))):
        taker[takes(sinks[e], pos)] = e
    return taker >= 0, taker


def counts(sinks, pos):
    """particles per sink under the first-sink attribution"""
    _, taker = attribute(sinks, pos)
    return [int((taker == e).sum()) for e in range(len(sinks))]


def renumber(remove):
    """(new_index, kept_from): new_index[i] = survivors in front of i (for every i), kept_from[j] = old index of new index j"""
    keep = np.asarray(remove).reshape(-1) == 0
    new_index = (np.cumsum(keep) - keep).astype(np.uint32)
    return new_index, np.flatnonzero(keep).astype(np.uint32)


def due(sink, s):
    """is the sink due in front of the substep whose substeps_done value is s?"""
    return s >= sink.start_substep and (s - sink.start_substep) % sink.period == 0


def due_sinks(sinks, s):
    """indices of the sinks evaluated in the one pass in front of substep s, in array order"""
    return [e for e, k in enumerate(sinks) if due(k, s)]


def firings(sink, substeps):
    """closed form: the passes the sink is due in, in front of substeps 0 .. substeps - 1"""
    if substeps <= sink.start_substep:
        return 0
    return (substeps - 1 - sink.start_substep) // sink.period + 1
