"""The slab exchange (kernels_shard.h: pack_face_body, rec_claim / rec_find; arrivals_body.inc; the leavers' list of g2p_body.inc) at every
capacity and wave boundary it compares a count with: scenes with exact counts, the rules in numpy, the case table (CPU only;
tests/test_shard_truth.py and tests/test_gpu_shard_boundaries.py assert, nothing here does).

The recipe is sort_truth's: F = I, no gravity, no colliders, SPEED cells per substep along x (the `mig-N` rows, placed by sort_truth._Placer,
also along y) — a group of particles that shares no node with a group of another velocity translates rigidly, so who crosses which cut in
which substep is set by where the particles start. A mover starts SPEED (K - 2) + SPEED / 2 cells in front of the cut and crosses it in
substep K - 1: its old owner's G2P of that substep lists it (Dev::leavers), it is the old owner's GUEST in substep K, travels in that
substep's message and is advanced and kept by its new owner. Ids are shuffled; positions keep 0.02 cells from every cell face (every
stencil weight is non-zero: whether a node pair is non-zero is decided by which cells hold particles), except where a row says a
coordinate is exact.

Geometry: cell c holds x / h in [c + 0.5, c + 1.5); the first cut is the lower x face of sort_truth.target_block — block 3 in 3D
(x / h = 12.5), block 2 in 2D (16.5); a middle slab is MIN_INTERIOR_WIDTH blocks wide.

Everything the truth says comes from two position snapshots (all particles, by id) and the SlabPartition:
  owner      the slab per particle (sharded.associated_block_x, the host's split)
  leavers    per face, the ids a slab's core lost in the substep between the snapshots: the migrants of the next message
  held       core + the leavers of the last substep: what stats()["num_particles"] and export() show
  halo_need  the (block, pair) records pack_face_body claims in the next message of a face"""
import collections
import functools
import itertools
import os
import re

import numpy as np

from oracle.np_oracle import assoc_cell, bw_of
from wgsparkl_amd import sharded
from wgsparkl_amd.sharded import SlabPartition, associated_block_x

from shard_oracle import iface_masks
from sort_truth import DT, H, K, SPEED, TARGETS, _Placer, _clump, _rng, _scene, target_block

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wgsparkl_amd", "csrc")
GENEROUS = 4096                       # the capacities of a row's twin: never reached by a row that passes


# ------------------------------------------------------------------------------------------------ the constants, from the sources
@functools.lru_cache(maxsize=None)
def constants(texts=None):
    """ARR_PER_WG (kernels_arrivals.h), MIN_INTERIOR_WIDTH (the refusal of wgs_shard_attach), LEAVERS_MIN and LEAVERS_DIV (Dev::leavers_cap
    = max(LEAVERS_MIN, particle_capacity / LEAVERS_DIV), capi_lifecycle.inc) and ARR_MAX_WGS (the arrivals' launch, host_substep.inc), read
    from the sources (`texts`: {file name: text} to parse instead)."""
    def text(name):
        if texts is not None:
            return texts[name]
        with open(os.path.join(_CSRC, name)) as f:
            return f.read()
    found = {}

    def take(names, name_of_file, pattern):
        m = re.findall(pattern, text(name_of_file))
        assert len(m) == 1, f"{names} not found exactly once in {name_of_file}: {m}"
        for n, v in zip(names, m[0] if isinstance(m[0], tuple) else (m[0],)):
            found[n] = int(v)
    take(("ARR_PER_WG",), "kernels_arrivals.h", r"\bconstexpr\s+int\s+ARR_PER_WG\s*=\s*(\d+)\s*;")
    take(("MIN_INTERIOR_WIDTH",), "capi_sharded.inc", r"has_lower && has_upper && \(int64_t\)d->dev\.shard_hi - \(int64_t\)d->dev\.shard_lo < (\d+)\)")
    take(("LEAVERS_MIN", "LEAVERS_DIV"), "capi_lifecycle.inc", r"leavers_cap = std::max<uint32_t>\((\d+)u, \(uint32_t\)\(c\.particle_capacity / (\d+)\)\)")
    take(("ARR_MAX_WGS",), "host_substep.inc", r"\(arr_most \+ ARR_PER_WG - 1u\) / ARR_PER_WG, (\d+)u\)")
    return found


_C = constants()
ARR_PER_WG, MIN_INTERIOR_WIDTH, LEAVERS_MIN, LEAVERS_DIV, ARR_MAX_WGS = (_C[k] for k in ("ARR_PER_WG", "MIN_INTERIOR_WIDTH", "LEAVERS_MIN", "LEAVERS_DIV", "ARR_MAX_WGS"))
WAVE = 64                             # the guests' copy hands out a face's slots per wave of 64 leavers; rec_claim looks at 64 slots at once


def leavers_cap(particle_capacity):
    return max(LEAVERS_MIN, particle_capacity // LEAVERS_DIV)


# ------------------------------------------------------------------------------------------------ the rules
def slab_of(part, rank):
    """(lo, hi, has_lower, has_upper) of a slab"""
    lo, hi = part.block_range(rank)
    return lo, hi, rank > 0, rank < part.world - 1


def owner(pos, part, dim):
    return part.owner_of_blocks(associated_block_x(np.asarray(pos, np.float32), H, dim))


def leavers(pos_a, pos_b, part, rank, dim):
    """(ids that left slab `rank`'s core through its lower face, through its upper face) in the substep pos_a -> pos_b, ascending"""
    oa, ob = owner(pos_a, part, dim), owner(pos_b, part, dim)
    mine = oa == rank
    return np.flatnonzero(mine & (ob < rank)), np.flatnonzero(mine & (ob > rank))


def held(pos_a, pos_b, part, rank, dim):
    """the ids slab `rank` holds at pos_b: those of its core that were its own one substep earlier, and the leavers of that substep — a
    particle that crossed into the core in the substep is still its old owner's guest (`pos_a` None: the start, nobody has moved)"""
    core = owner(pos_b, part, dim) == rank
    if pos_a is None:
        return np.flatnonzero(core)
    stayed = np.flatnonzero(core & (owner(pos_a, part, dim) == rank))
    return np.sort(np.concatenate((stayed,) + leavers(pos_a, pos_b, part, rank, dim)))


def _offsets(dim, width):
    return np.asarray(list(itertools.product(range(width), repeat=dim)), np.int64)


def halo_need(pos, ids, part, rank, face, dim, regular=True):
    """The records of the message slab `rank`, holding the particles `ids` at `pos`, sends through `face` (0 lower, 1 upper): the set of
    (block coordinates, pair). kernels_sort.h lists the active blocks of the layers with a send mask (a block with particles and its
    "+" neighbours are active); pack_face_body claims, per listed block and pair of the mask, a record when the pair is `regular` —
    pair 0 of layer lo / hi, which every core particle near the face writes — or when one of its nodes is non-zero: some held particle's
    3^D stencil (the nodes c .. c + 2 of its associated cell c) reaches it. (`regular` False: the rule without the first clause — a
    fault the tests inject.)"""
    bw, ntag = bw_of(dim), bw_of(dim) // 2
    lo, hi, has_lo, has_hi = slab_of(part, rank)
    if not (has_lo if face == 0 else has_hi) or len(ids) == 0:
        return set()
    cell = assoc_cell(np.asarray(pos, np.float32)[ids], H)
    active = np.unique((np.unique(cell // bw, axis=0)[:, None, :] + _offsets(dim, 2)[None, :, :]).reshape(-1, dim), axis=0)
    out = set()
    for b in active:
        send = iface_masks(int(b[0]), lo, hi, has_lo, has_hi, ntag)[1 + face]
        for t in range(ntag):
            if not (send >> t) & 1:
                continue
            is_regular = regular and t == 0 and int(b[0]) == (lo if face == 0 else hi)
            if not is_regular:
                first = b * bw
                first[0] += 2 * t                                   # the pair's nodes: x in [first, first + 1], the other axes the whole block
                last = b * bw + (bw - 1)
                last[0] = first[0] + 1
                if not ((cell <= last) & (cell + 2 >= first)).all(1).any():
                    continue
            out.add((tuple(int(x) for x in b), t))
    return out


def off_faces(pos):
    """the distance of every coordinate from the nearest cell face, in cells"""
    f = (np.asarray(pos, np.float64) / H - 0.5) % 1.0
    return np.minimum(f, 1.0 - f)


def facts(part, dim, pos_a, pos_b):
    """what the substep after pos_b meets, per slab: leavers[(slab, face)] and held[slab] (ids), halo[(slab, face)] (records)"""
    out = dict(leavers={}, held=[], halo={})
    for r in range(part.world):
        mine = held(pos_a, pos_b, part, r, dim)
        out["held"].append(mine)
        lv = leavers(pos_a, pos_b, part, r, dim) if pos_a is not None else (np.zeros(0, np.int64),) * 2
        for f in (0, 1):
            if len(lv[f]):
                out["leavers"][(r, f)] = lv[f]
            need = halo_need(pos_b, mine, part, r, f, dim)
            if need:
                out["halo"][(r, f)] = need
    return out


def counts(fx):
    """facts() as the numbers a row spells: ({(slab, face): leavers}, [held per slab], {(slab, face): records})"""
    return {k: len(v) for k, v in fx["leavers"].items()}, [len(h) for h in fx["held"]], {k: len(v) for k, v in fx["halo"].items()}


# ------------------------------------------------------------------------------------------------ builders
def first_cut(dim):
    return target_block(dim)[0]


def partition(dim, world):
    """cuts: the first at first_cut, a middle slab MIN_INTERIOR_WIDTH blocks wide (the ends are open)"""
    b = first_cut(dim)
    return SlabPartition([b - 64] + [b + MIN_INTERIOR_WIDTH * r for r in range(world - 1)] + [b + 64 + MIN_INTERIOR_WIDTH * world])


class _Cloud:
    """groups of particles, each with its own velocity of s * SPEED cells per substep along x (s in -1, 0, 1)"""

    def __init__(self, dim, rng):
        self.dim, self.bw, self.rng, self.pos, self.s = dim, bw_of(dim), rng, [], []
        self.yz = tuple(np.asarray(target_block(dim))[1:] * self.bw + 1)        # the row of cells everything sits in unless told otherwise

    def _add(self, pos, s):
        self.pos.append(np.asarray(pos, np.float64).reshape(-1, self.dim))
        self.s.append(np.full(len(self.pos[-1]), s, np.int64))

    def residents(self, cx, s, n, yz=None):
        """`n` particles that stay in cell (cx, yz) for K substeps of motion s"""
        yz = self.yz if yz is None else yz
        u = self.rng.uniform(0.05, 0.70, n)
        p = np.empty((n, self.dim))
        p[:, 0] = cx + 0.5 + (1.0 - u if s < 0 else u)
        for k in range(1, self.dim):
            p[:, k] = yz[k - 1] + 0.5 + self.rng.uniform(0.1, 0.9, n)
        self._add(p, s)

    def movers(self, block, s, n, cells=None, at=K - 1):
        """`n` particles that cross the lower x face of block layer `block` in direction s in substep `at`, spread over the (y, z) `cells`"""
        cells = [self.yz] if cells is None else cells
        face = block * self.bw + 0.5
        d0 = SPEED * (at - 1) + SPEED / 2
        for i, yz in enumerate(cells):
            m = n // len(cells) + (1 if i < n % len(cells) else 0)
            if m:
                self._add(_clump((face - s * d0,) + tuple(c + 1.0 for c in yz), m, self.rng), s)

    def points(self, pts, s=0):
        self._add(pts, s)

    def scene(self, grid_capacity=1024):
        pos, s = np.concatenate(self.pos), np.concatenate(self.s)
        order = self.rng.permutation(len(pos))          # ids in no order: the order by id is not the storage order
        sc = _scene(pos[order], (0.0,) * self.dim)
        sc["particles"].vel[:, 0] = (s[order] * SPEED * (H / DT)).astype(np.float32)
        sc["grid_capacity"] = grid_capacity
        return sc


def designed(sc, k):
    """the positions after `k` substeps of pure translation (what the oracle and the device reproduce to round-off)"""
    ps = sc["particles"]
    return (ps.pos.astype(np.float64) + k * ps.vel.astype(np.float64) * DT).astype(np.float32)


def mig_scene(dim, n):
    """`n` movers from slab 0 into slab 1 (sort_truth._Placer: the arrivals of local cell 24 of the target block), residents on both sides"""
    t = TARGETS[dim][24]
    p = _Placer(dim, t, _rng("shard-mig", dim, n))
    p.enter_x(t, n)
    p.residents((1,) + t[1:], 6)
    p.residents((-3,) + t[1:], 6)          # (three cells below the cut: the block layer of slab 0 at the face)
    return _scene(p.positions(), p.velocity)


def cross_scene(dim, up=0, down=0, wide=False):
    """two slabs: `up` movers from slab 0 into slab 1, `down` movers the other way one block row further along y (no node in common with
    the first group: each translates rigidly), residents around each group. `wide`: the movers over 16 x 16 (y, z) cells, as a sheet."""
    c = _Cloud(dim, _rng("shard-cross", dim, up, down, wide))
    x0 = first_cut(dim) * c.bw
    cells = [(c.yz[0] + i, c.yz[1] + j) for i in range(16) for j in range(16)] if wide else None
    c.residents(x0 - 3, 1, 6)
    c.residents(x0 + 1, 1, 6)
    c.movers(first_cut(dim), 1, up, cells)
    if down:
        far = (c.yz[0] + 2 * c.bw,) + c.yz[1:]
        c.residents(x0 - 3, -1, 4, far)
        c.residents(x0 + 1, -1, 4, far)
        c.movers(first_cut(dim), -1, down, [far])
    return c.scene()


def middle_scene(dim, out=(0, 0), into=(0, 0), wide=False):
    """three slabs; the middle one loses out[0] particles through its lower and out[1] through its upper face and receives into[0] from
    below and into[1] from above, all in the same substep. The four groups share no node: the two faces are MIN_INTERIOR_WIDTH blocks
    apart, and those that come in sit two block rows further along y than those that go out."""
    c = _Cloud(dim, _rng("shard-middle", dim, out, into, wide))
    lo, hi = first_cut(dim), first_cut(dim) + MIN_INTERIOR_WIDTH
    far = (c.yz[0] + 2 * c.bw,) + c.yz[1:]
    cells_far = [(far[0] + i, far[1] + j) for i in range(16) for j in range(16)] if wide else [far]
    for block, s, n, yz, cells in ((lo, -1, out[0], c.yz, None), (hi, 1, out[1], c.yz, None), (lo, 1, into[0], far, cells_far), (hi, -1, into[1], far, cells_far)):
        face_cell = block * c.bw
        c.residents(face_cell - 3, s, 4, yz)
        c.residents(face_cell + 2, s, 4, yz)
        c.movers(block, s, n, cells)
    return c.scene()


def face_scene(dim, my, mz=1):
    """two slabs, static counts: one particle per block in the last cell layer below the cut and one in the first above it, over `my` x `mz`
    blocks of the face. Each message holds the regular pair of every active block of its layer — (my + 1)(mz + 1) records in 3D, my + 1
    in 2D (a block's "+" neighbours are active) — and nothing else: the particles sit in the middle of their block along y and z."""
    c = _Cloud(dim, _rng("shard-face", dim, my, mz))
    x0 = first_cut(dim) * c.bw
    for by in range(my):
        for bz in range(mz if dim == 3 else 1):
            yz = ((target_block(dim)[1] + by) * c.bw + 1, (target_block(dim)[-1] + bz) * c.bw + 1)[:dim - 1]
            c.residents(x0 - 1, 1, 1, yz)
            c.residents(x0, 1, 1, yz)
    return c.scene()


def growing_scene(dim):
    """two slabs, 6 substeps, everything about the LOWER message (slab 1 to slab 0). A face of 3 block rows, static. Further along y, each
    in a block row of its own: a group that leaves the face layer for the layer above it in substep 2 (its blocks drop out of the message
    of substep 3) while another enters the face layer from above (two or four new blocks in that message: fresh claims beside records
    that keep their slot by the steady-state shortcut); and a group that crosses the cut in substep 3 and, as slab 1's guests in substep 4,
    makes a pair of layer lo - 1 non-zero that only guests reach: the message of substep 4 is the fullest of the run."""
    c = _Cloud(dim, _rng("shard-growing", dim))
    x0 = first_cut(dim) * c.bw
    row = lambda r: ((target_block(dim)[1] + r) * c.bw + 1,) + c.yz[1:]
    for r in range(3):
        c.residents(x0 - 1, 1, 2, row(r))
        c.residents(x0, 1, 2, row(r))
    c.movers(first_cut(dim) + 1, 1, 3, [row(5)], at=2)
    c.movers(first_cut(dim) + 1, -1, 3, [row(8)], at=2)
    c.movers(first_cut(dim), -1, 2, [row(11)], at=3)
    return c.scene()


def cut_scene(dim, mover):
    """No motion: particles at the x where associated_block_x flips from slab 0 to slab 1, at the float32 below and above it, a few at
    either side; with `mover` one particle more, alone in its block row, that lands exactly on that x after one substep."""
    c = _Cloud(dim, _rng("shard-cut", dim, mover))
    flip = np.float32(first_cut(dim) * c.bw + 0.5)
    mid = tuple(v + 1.0 for v in c.yz)
    xs = [np.nextafter(flip, np.float32(-np.inf)), flip, np.nextafter(flip, np.float32(np.inf))]
    pts = [(float(x),) + tuple(m + 0.1 * i for m in mid) for i, x in enumerate(xs) for _ in range(2)]
    c.points(pts)
    c.residents(first_cut(dim) * c.bw - 2, 0, 4)
    c.residents(first_cut(dim) * c.bw + 1, 0, 4)
    sc = c.scene()
    if mover:
        ps = sc["particles"]
        far = tuple(v + 3 * c.bw + 1.0 for v in c.yz)
        start, vel = float(flip) - 0.0625, 0.0625 * H / DT
        i = int(np.argmin(np.abs(ps.pos[:, 0] - (first_cut(dim) * c.bw - 1.0))))      # one of the residents below the cut becomes the mover
        ps.pos[i] = (start,) + far
        ps.vel[i, 0] = vel
    return sc


def flip_x(dim):
    return np.float32(first_cut(dim) * bw_of(dim) + 0.5)


# ------------------------------------------------------------------------------------------------ the case table
# One row per case and dimension.
#   build      (builder, keyword arguments); world: the number of slabs; substeps: K — the checked substep, the one whose messages carry the
#              leavers of substep K - 1 (pos_a: after K - 2 substeps, pos_b: after K - 1)
#   leavers    {(slab, face): count} of substep K - 1; held: particles per slab after it; halo: {(slab, face): records} of substep K's messages
#   caps       halo_capacity_records / migrant_capacity of the group, and particle_capacity per slab (None: room for the whole scene), spelled
#              relative to the row's own counts
#   over       None, or (the substep in which the overflow happens, the slabs that report it)
Row = collections.namedtuple("Row", "name family dim build world substeps leavers held halo halo_cap mig_cap capacity over exact")
ROWS = []


def _add(name, family, dim, builder, kw, world, leavers, held, halo, halo_cap=None, mig_cap=None, capacity=None, over=None, substeps=K, exact=False):
    ROWS.append(Row(f"{name}-{dim}d", family, dim, (builder, dict(kw, dim=dim)), world, substeps, leavers, held, halo, halo_cap, mig_cap, capacity,
                    over, exact))


def _both(dim):
    return 2 if dim == 2 else 4        # the records of a one-block face: the block and its "+" neighbours along y (and z)


for _d in (3, 2):
    _h = {(0, 1): _both(_d), (1, 0): _both(_d)}
    # with guests of slab 0 above the cut: the second pair of their block (and, where they reach the next block row along y, of that one)
    _hg = {(0, 1): _both(_d) + (2 if _d == 3 else 1), (1, 0): _both(_d)}          # placed by _Placer: local cell (0, 2, 1) / (0, 3)
    _hc = {(0, 1): _both(_d) + 1, (1, 0): _both(_d)}                              # placed by _Cloud: the middle of the block along y and z
    # ---- mig-N: the leavers of one substep through one face
    for _n in (0, 1, ARR_PER_WG - 1, ARR_PER_WG, ARR_PER_WG + 1, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE, 2 * WAVE + 1):
        _add(f"mig-{_n}", "mig", _d, mig_scene, dict(n=_n), 2, {(0, 1): _n} if _n else {}, [6 + _n, 6], _hg if _n else _h, halo_cap=2 * _both(_d) + 7, mig_cap=_n + 3)
    # ---- migrant_capacity exactly reached, and one more
    for _n in (1, WAVE, WAVE + 1):
        _add(f"migcap-at-{_n}", "migcap", _d, cross_scene, dict(up=_n), 2, {(0, 1): _n}, [6 + _n, 6], _hc, mig_cap=_n)
        _m = _n + 1 if _n == 1 else _n          # (a capacity of 0 is refused by wgs_shard_attach: one more leaver instead of one slot less)
        _add(f"migcap-over-{_n}", "migcap", _d, cross_scene, dict(up=_m), 2, {(0, 1): _m}, [6 + _m, 6], _hc, mig_cap=_m - 1, over=(K, (0,)))
    # ---- both faces of a middle slab in one substep, and arrivals from both messages in the same substep
    _hm = {k: 2 * _both(_d) + 1 for k in ((0, 1), (1, 0), (1, 1), (2, 0))}
    for _a, _b in ((1, 1), (5, 3), (31, 33), (64, 64)):
        _add(f"mig-both-{_a}+{_b}", "mig-both", _d, middle_scene, dict(out=(_a, _b), into=(_a, _b)), 3, {(1, 0): _a, (1, 1): _b, (0, 1): _a, (2, 0): _b},
             [8 + _a, 16 + _a + _b, 8 + _b], _hm, halo_cap=4 * _both(_d) + 3, mig_cap=max(_a, _b))
    # ---- room: the particle capacity of the receiver exactly filled by the arrivals, and one short
    for _g in (0, 2):
        _kw = dict(up=5, down=_g)
        _lv = {(0, 1): 5, (1, 0): _g} if _g else {(0, 1): 5}
        _hr = {(0, 1): 2 * _both(_d) + 1, (1, 0): 2 * _both(_d) + 1} if _g else _hc
        _held = [6 + 5 + (4 if _g else 0), 6 + (4 + _g if _g else 0)]
        _tag = f"-{_g}-guests" if _g else ""
        _add(f"room-at{_tag}", "room", _d, cross_scene, _kw, 2, _lv, _held, _hr, capacity=(None, _held[1] + 5))
        _add(f"room-over{_tag}", "room", _d, cross_scene, _kw, 2, _lv, _held, _hr, capacity=(None, _held[1] + 4), over=(K, (1,)))
    # ---- on the cut
    _add("on-the-cut", "cut", _d, cut_scene, dict(mover=False), 2, {}, [2 + 2 + 4, 2 + 4], _h, substeps=1, exact=True)
    _add("on-the-cut-mover", "cut", _d, cut_scene, dict(mover=True), 2, {}, [2 + 2 + 4, 2 + 4], {(0, 1): 2 * _both(_d), (1, 0): _both(_d)}, substeps=2, exact=True)
    # ---- a message's table exactly full, and one record short: 1 .. 64 + 1 .. 2 * 64 + 2 records, faces of more than one block
    for _need, (_my, _mz) in {_both(_d): (1, 1), 63: (8, 6), 64: (7, 7), 65: (12, 4), 130: (12, 9)}.items():
        if _d == 2:
            _my, _mz = _need - 1, 1
        _hf = {(0, 1): _need, (1, 0): _need}
        _n = _my * _mz
        _add(f"halo-at-{_need}", "halo", _d, face_scene, dict(my=_my, mz=_mz), 2, {}, [_n, _n], _hf, halo_cap=_need)
        _add(f"halo-over-{_need}", "halo", _d, face_scene, dict(my=_my, mz=_mz), 2, {}, [_n, _n], _hf, halo_cap=_need - 1, over=(1, (0, 1)))
# ---- the leavers' list (3D): 4096 entries whatever the capacity below 16 x 4097
for _n in (LEAVERS_MIN - 1, LEAVERS_MIN, LEAVERS_MIN + 1):
    _add(f"leavers-{_n}", "leavers", 3, cross_scene, dict(up=_n, wide=True), 2, {(0, 1): _n}, [6 + _n, 6], {(0, 1): 61, (1, 0): 4}, mig_cap=LEAVERS_MIN + 104,
         over=(K - 1, (0,)) if _n > LEAVERS_MIN else None)
# ---- the arrivals' grid-stride loop (3D): one arrival more than ARR_MAX_WGS workgroups of ARR_PER_WG take in one trip
_NS = ARR_MAX_WGS * ARR_PER_WG // 2
_add("arrivals-stride", "stride", 3, middle_scene, dict(into=(_NS, _NS + 1), wide=True), 3, {(0, 1): _NS, (2, 0): _NS + 1}, [8 + _NS, 16, 8 + _NS + 1],
     {(0, 1): 65, (1, 0): 8, (1, 1): 8, (2, 0): 65}, mig_cap=LEAVERS_MIN + 104, capacity=(LEAVERS_DIV * (LEAVERS_MIN + 200),) * 3)
# ---- a full table over six substeps while the face grows: the steady-state shortcut beside fresh claims
for _d in (3, 2):
    _add("halo-steady-and-new", "growing", _d, growing_scene, {}, 2, {}, [8, 12], {(0, 1): 3 * _both(_d), (1, 0): 3 * _both(_d)}, halo_cap="max", substeps=6)
# the records of the lower message of halo-steady-and-new, substep by substep: steady, steady, two blocks out and two in, the guests' pair, less
GROWING_LOWER = {_d: [4 * _both(_d)] * 3 + [4 * _both(_d) + 1] + [3 * _both(_d)] * 2 for _d in (3, 2)}

ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS), "two rows of one name"


def build(row):
    builder, kw = row.build
    return builder(**kw)


def part_of(row):
    return partition(row.dim, row.world)


def needs_over_time(row, sc=None):
    """[{(slab, face): records}] of the messages of substeps 1 .. row.substeps, from the designed positions"""
    sc = build(row) if sc is None else sc
    part = part_of(row)
    out = []
    for k in range(1, row.substeps + 1):
        pos_a = designed(sc, k - 2) if k >= 2 else None
        out.append(counts(facts(part, row.dim, pos_a, designed(sc, k - 1)))[2])
    return out


def capacities(row, sc=None):
    """(halo_capacity_records, migrant_capacity, [particle_capacity per slab]) of the row; ("max": the most records a message of the run holds)"""
    sc = build(row) if sc is None else sc
    halo = row.halo_cap
    if halo == "max":
        halo = max(max(n.values()) for n in needs_over_time(row, sc))
    cap = [sc["particles"].n] * row.world
    if row.capacity is not None:
        cap = [sc["particles"].n if c is None else c for c in row.capacity]
    return GENEROUS if halo is None else halo, GENEROUS if row.mig_cap is None else row.mig_cap, cap


def check_facts(row, pos_a, pos_b, fx=None, held_ids=None):
    """facts() equals the row, count by count (==); `held_ids`: what each slab itself says it holds (export()["ids"]) — equal to the truth's
    set. Returns the facts."""
    part = part_of(row)
    fx = facts(part, row.dim, pos_a, pos_b) if fx is None else fx
    lv, hd, halo = counts(fx)
    if row.leavers is not None:
        assert lv == row.leavers, f"{row.name}: leavers {lv}, designed {row.leavers}"
    if row.held is not None:
        assert hd == row.held, f"{row.name}: held {hd}, designed {row.held}"
    if row.halo is not None:
        assert halo == row.halo, f"{row.name}: halo records {halo}, designed {row.halo}"
    if held_ids is not None:
        for r, ids in enumerate(held_ids):
            got = np.sort(np.asarray(ids, np.int64))
            assert np.array_equal(got, fx["held"][r]), f"{row.name}: slab {r} holds {len(got)} particles, the truth {len(fx['held'][r])}: " \
                f"only the slab {np.setdiff1d(got, fx['held'][r])[:10].tolist()}, only the truth {np.setdiff1d(fx['held'][r], got)[:10].tolist()}"
    return fx
