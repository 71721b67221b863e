"""The regrouping thresholds of the sort (kernels_sort.h, launch 2: regroup_block; launch 1 of a rebuild: bin_body), each met at its exact value
and one to either side (CPU only; tests/test_sort_truth.py and tests/test_gpu_sort_boundaries.py assert, nothing here does).

Three things live here:
  * the scene recipe test_gpu_sort_order.py introduced (`_scene`, `_clump`, `facts`, `_lexsorted_runs`): particles with F = I, one velocity
    and no gravity translate rigidly, so who crosses which cell face in which substep is set by where the particles start;
  * builders that take the counts a predicate of the kernel compares — previous run, arrivals, changers, the members of one cell — and
    place residents, clumps of movers and leavers so that the sort of substep K meets exactly those counts;
  * `paths`, the kernel's predicates restated in numpy from the positions before and after the motion the sort meets, and the case table
    `ROWS`, one row per boundary case with the designed counts and the outcome of every predicate spelled out.

The constants are read from kernels_sort.h and layout.h: a change in the kernel moves the cases with it.

Geometry: cell c holds x / h in [c + 0.5, c + 1.5) (oracle.np_oracle.assoc_cell); the target block T is (3, 2, 2) in 3D (BW = 4) and (2, 2)
in 2D (BW = 8). Everybody moves 0.05 cells per substep along x and y (the signs are the scene's: they decide through which face a cell is
entered), nobody along z. A resident keeps 0.05 .. 0.70 of a cell behind it (counted against the motion) and so stays in its cell for all
K = 4 substeps; a mover starts 0.05 (K - 2) + 0.025 cells in front of the face it is to cross and crosses it in substep K - 1."""
import collections
import functools
import os
import re
import zlib

import numpy as np

from wgsparkl_amd.models import MODEL_NEO_HOOKEAN, ElasticCoefficients, ParticlePhase
from wgsparkl_amd.solver import ParticleSet, SimulationParams

from oracle.np_oracle import assoc_cell, bw_of

H, DT = 1.0, 1.0e-3
K = 4                  # substeps of a steady-state case; the sort of substep K meets the motion of substep K - 1
SPEED = 0.05           # cells per substep
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wgsparkl_amd", "csrc")
_NAMES = ("RUNCAP", "BLK_ARR", "ARRC", "NEWC", "PAR_R", "TOUCH_SET", "SORT_THREADS", "NPB")


@functools.lru_cache(maxsize=None)
def constants(text=None):
    """{name: value} of _NAMES, from the `constexpr` definitions of kernels_sort.h and layout.h (`text`: a copy to parse instead). An
    initialiser may name constants defined before it (PAR_R = (RUNCAP + 63) / 64); the division is C's."""
    if text is None:
        text = ""
        for name in ("layout.h", "kernels_sort.h"):
            with open(os.path.join(_CSRC, name)) as f:
                text += f.read() + "\n"
    out = {}
    for name, expr in re.findall(r"\bconstexpr\s+(?:int|uint32_t)\s+(\w+)\s*=\s*([^;]+);", text):
        if name not in _NAMES:
            continue
        expr = re.sub(r"\b(\d+)u\b", r"\1", expr).replace("/", "//")
        assert re.fullmatch(r"[\w\s()+\-*/]+", expr), f"{name}: an initialiser this parser cannot read: {expr}"
        value = int(eval(expr, {"__builtins__": {}}, dict(out)))    # (digits, names parsed above, + - * // and parentheses only)
        assert out.get(name, value) == value, f"{name} is defined twice with different values"
        out[name] = value
    missing = [n for n in _NAMES if n not in out]
    assert not missing, f"not found in the headers: {missing}"
    return out


_C = constants()
RUNCAP, BLK_ARR, ARRC, NEWC, PAR_R = _C["RUNCAP"], _C["BLK_ARR"], _C["ARRC"], _C["NEWC"], _C["PAR_R"]
TOUCH_SET, SORT_THREADS, NPB = _C["TOUCH_SET"], _C["SORT_THREADS"], _C["NPB"]
HALF = 64 * (PAR_R // 2)       # a staged run longer than this needs the second staging batch


# ------------------------------------------------------------------------------------------------ the recipe of test_gpu_sort_order.py
def _scene(pos, cells_per_substep, colliders=()):
    pos = np.asarray(pos, np.float32)
    dim = pos.shape[1]
    ps = ParticleSet.uniform(pos, H / 4.0, 1000.0, ElasticCoefficients.from_young_modulus(1.0e3, 0.3), phase=ParticlePhase(1.0, -1.0))
    ps.vel[:] = (np.asarray(cells_per_substep, np.float64) * (H / DT)).astype(np.float32)
    return dict(particles=ps, params=SimulationParams(gravity=(0.0,) * dim, dt=DT), colliders=list(colliders), cell_width=H,
                grid_capacity=1024, model=MODEL_NEO_HOOKEAN)


def _clump(centre, count, rng, spread=0.004):
    return np.asarray(centre) * H + rng.uniform(-spread, spread, (count, len(centre))) * H


def local_key(cell, dim):
    """the in-block cell t0 + (t1 << BSHIFT) + (t2 << 2 BSHIFT) of world cells: the lane that owns the cell"""
    bw = bw_of(dim)
    bshift = bw.bit_length() - 1
    t = np.asarray(cell) % bw
    return sum(t[..., k] << (bshift * k) for k in range(dim))


def facts(pos_a, pos_b, dim):
    """What the sort that orders `pos_b` meets; `pos_a`: the positions one substep earlier (None: the first substep)."""
    bw = bw_of(dim)
    cb = assoc_cell(pos_b, H)
    cells, inv, per_cell = np.unique(cb, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    blocks, binv, per_block = np.unique(cb // bw, axis=0, return_inverse=True, return_counts=True)
    binv = binv.reshape(-1)
    f = dict(per_cell=per_cell, per_block=per_block, dim=dim, cell_a=None, cell_b=cb)
    if pos_a is not None:
        ca = assoc_cell(pos_a, H)
        moved = (ca != cb).any(1)
        hopped = (ca // bw != cb // bw).any(1)
        f["cell_a"] = ca
        f["changed_cell_in_block"] = int((moved & ~hopped).sum())
        f["changed_block"] = int(hopped.sum())
        f["new_same"] = np.bincount(inv[moved & ~hopped], minlength=len(cells))     # newcomers per cell, from its own block ...
        f["new_other"] = np.bincount(inv[hopped], minlength=len(cells))             # ... and from other blocks
        f["arrivals"] = np.bincount(binv[hopped], minlength=len(blocks))            # per block, from other blocks
        f["prev_run"] = np.unique(ca // bw, axis=0, return_counts=True)[1]          # the blocks' previous runs
    return f


def _lexsorted_runs(pos, dim):
    """read_blocks() of an orderer that is right by construction: (vid, first, num, ids) of the canonical order of `pos`"""
    bw = bw_of(dim)
    c = assoc_cell(pos, H)
    blocks, binv, num = np.unique(c // bw, axis=0, return_inverse=True, return_counts=True)
    ids = np.lexsort((np.arange(len(pos)), local_key(c, dim), binv.reshape(-1)))
    return blocks, np.concatenate([[0], np.cumsum(num)[:-1]]), num, ids


# ------------------------------------------------------------------------------------------------ the kernel's predicates
Paths = collections.namedtuple("Paths", "runlen narr btotal dirty in_lds par out_lds second_half on_lists stayed new_same new_other total "
                                        "tail network cached coop select")


def paths(f, block):
    """The predicates of regroup_block for `block` (world block coordinates), from facts(): what the wave that regroups it compares.
      runlen        its previous run: the particles that were in it before the motion (0 on a rebuild substep: no previous run is used)
      narr          arrivals from other blocks (push_arrival counts them in blk_narr; 0 on a rebuild substep: bin_body lists everybody)
      btotal        its new run
      dirty         a particle of the previous run changed cell (block_dirty)
      in_lds        runlen <= RUNCAP
      on_lists      somebody is on a cell's list: narr > BLK_ARR (the array holds the first BLK_ARR), or a rebuild substep with particles
      par           the wave-parallel form: steady state (of a block that was active one substep ago: a block without a previous run
                    that the kernel can use — new, or back after a pause — takes the lane form whatever this says), something to do
                    (dirty or arrivals), in_lds, nobody on a list and runlen + min(narr, BLK_ARR) <= RUNCAP
      second_half   the second staging batch runs: the run is staged (in_lds, something to do) and runlen > 64 (PAR_R / 2)
      out_lds       btotal <= RUNCAP
      tail          runlen % 64: the entries of the last, partly filled round of a staged run (0: it ends on a full round)
    and per in-block cell (arrays of NPB, lane = cell):
      stayed, new_same, new_other, total   members that did not change cell / came from a cell of this block / from another block / all
      network       par form: the cell orders its newcomers in ONE batch of the register network (at most NEWC of them)
      cached        lane form: the cell's arrivals fit the registers (at most ARRC; hand_over keeps the first ARRC in LDS)
      coop          lane form, more than ARRC arrivals: the whole wave orders the cell (both stages in LDS and total <= 64)
      select        lane form, more than ARRC arrivals and not coop: smallest-key selection (next_arrival)"""
    dim, cb, ca = f["dim"], f["cell_b"], f["cell_a"]
    bw = bw_of(dim)
    block = np.asarray(block, np.int64)
    in_b = (cb // bw == block).all(1)
    key = local_key(cb, dim)
    count = lambda sel: np.bincount(key[sel], minlength=NPB)
    btotal = int(in_b.sum())
    total = count(in_b)
    zero = np.zeros(NPB, np.int64)
    if ca is None:
        steady, runlen, narr, dirty = False, 0, 0, False
        stayed, new_same, new_other = zero, zero, total
        on_lists = btotal > 0
    else:
        steady = True
        in_a = (ca // bw == block).all(1)
        moved = (ca != cb).any(1)
        runlen, narr = int(in_a.sum()), int((in_b & ~in_a).sum())
        dirty = bool((in_a & moved).any())
        stayed, new_same, new_other = count(in_b & ~moved), count(in_b & in_a & moved), count(in_b & ~in_a)
        on_lists = narr > BLK_ARR
    in_lds = runlen <= RUNCAP
    need_ids = dirty or narr > 0 or on_lists
    par = steady and need_ids and in_lds and not on_lists and runlen + min(narr, BLK_ARR) <= RUNCAP
    second_half = in_lds and need_ids and runlen > HALF
    out_lds = btotal <= RUNCAP
    new = new_same + new_other
    many = ~par & (new > ARRC)
    coop = many & (in_lds and out_lds) & (total <= 64)
    return Paths(runlen, narr, btotal, dirty, in_lds, par, out_lds, second_half, on_lists, stayed, new_same, new_other, total,
                 runlen % 64, par & (new <= NEWC), ~par & (new <= ARRC), coop, many & ~coop)


def workgroup_blocks(pos, dim):
    """distinct blocks per workgroup of launch 1 of a rebuild substep (bin_body: SORT_THREADS consecutive particles of the caller's order)"""
    b = assoc_cell(np.asarray(pos, np.float32), H) // bw_of(dim)
    return [len(np.unique(b[i:i + SORT_THREADS], axis=0)) for i in range(0, len(b), SORT_THREADS)]


# ------------------------------------------------------------------------------------------------ builders
def target_block(dim):
    return (3, 2, 2) if dim == 3 else (2, 2)


def _cell_of_key(key, dim):
    bw = bw_of(dim)
    bs = bw.bit_length() - 1
    return tuple((key >> (bs * k)) & (bw - 1) for k in range(dim))


def _key_of_cell(t, dim):
    bs = bw_of(dim).bit_length() - 1
    return sum(int(t[k]) << (bs * k) for k in range(dim))


TARGETS = {3: {0: (0, 0, 0), 24: (0, 2, 1), 63: (3, 3, 3)}, 2: {0: (0, 0), 24: (0, 3), 63: (7, 7)}}     # local cell -> its coordinates


class _Placer:
    """positions in the target block of one scene: `sx`, `sy` the signs of the motion along x and y"""

    def __init__(self, dim, target, rng):
        self.dim, self.bw, self.rng = dim, bw_of(dim), rng
        self.t = tuple(target)
        assert self.t[0] in (0, self.bw - 1), "a cell that another block's particles enter across an x face lies in the first or last x layer"
        self.sx = 1 if self.t[0] == 0 else -1
        self.sy = 1 if self.t[1] > 0 else -1
        self.lo = np.asarray(target_block(dim)) * self.bw + 0.5        # x / h of the block's lower corner
        self.d = SPEED * (K - 2) + SPEED / 2                           # a mover's start in front of its face
        self.parts = []

    @property
    def velocity(self):
        return (SPEED * self.sx, SPEED * self.sy, 0.0)[:self.dim]

    def _rest(self, cell):
        """the place of a clump that only rides along in local cell `cell`: 0.4 of a cell behind it on the moving axes, mid-cell along z"""
        off = [0.4 if self.sx > 0 else 0.6, 0.4 if self.sy > 0 else 0.6, 0.5][:self.dim]
        return self.lo + np.asarray(cell) + np.asarray(off)

    def residents(self, cell, n):
        if n == 0:
            return
        u = self.rng.uniform(0.05, 0.70, (n, self.dim))
        for k, s in ((0, self.sx), (1, self.sy)):
            if s < 0:
                u[:, k] = 1.0 - u[:, k]
        if self.dim == 3:
            u[:, 2] = self.rng.uniform(0.1, 0.9, n)
        self.parts.append(self.lo + np.asarray(cell) + u)

    def enter_x(self, cell, n):
        """`n` particles that enter local cell `cell` from the neighbouring block across its x face"""
        if n == 0:
            return
        assert cell[0] == self.t[0]
        c = self._rest(cell)
        face = self.lo[0] + (0 if self.sx > 0 else self.bw)
        c[0] = face - self.sx * self.d
        self.parts.append(_clump(c, n, self.rng))

    def leave_x(self, cell, n):
        """`n` particles of local cell `cell` that leave the block across the opposite x face"""
        if n == 0:
            return
        assert cell[0] == (self.bw - 1 if self.sx > 0 else 0)
        c = self._rest(cell)
        face = self.lo[0] + (self.bw if self.sx > 0 else 0)
        c[0] = face - self.sx * self.d
        self.parts.append(_clump(c, n, self.rng))

    def enter_y(self, cell, n):
        """`n` particles that enter local cell `cell` across a y face from the cell behind it, which lies in the block; returns that cell"""
        src = list(cell)
        src[1] -= self.sy
        assert 0 <= src[1] < self.bw
        if n:
            c = self._rest(cell)
            face = self.lo[1] + cell[1] + (0 if self.sy > 0 else 1)
            c[1] = face - self.sy * self.d
            self.parts.append(_clump(c, n, self.rng))
        return tuple(src)

    def positions(self):
        pos = np.concatenate(self.parts)
        return pos[self.rng.permutation(len(pos))]       # ids in no order: newcomers rank among the stayers, not behind them


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _spread(n, cells, fixed):
    """`n` residents over `cells` as evenly as it goes (the first cells take the remainder); `fixed`: {cell: count} taken as given"""
    free = [c for c in cells if c not in fixed]
    n -= sum(fixed.values())
    assert n >= 0 and (free or n == 0)
    out = dict(fixed)
    for i, c in enumerate(free):
        out[c] = n // len(free) + (1 if i < n % len(free) else 0)
    return out


def steady_scene(dim, R, A=0, changers=3, leavers=0, cell=24, triple=None, arr_cells=1, big=0, changers_last=False):
    """A scene whose sort of substep K meets, in the target block: a previous run of `R`; `A` arrivals from the neighbouring block, which
    holds nothing else, into local cell `cell` (`arr_cells` = 2: half of them into a second cell); `changers` particles that change cell
    inside the block, away from `cell` (`changers_last`: out of the last cell of the previous run, which holds nobody else); `leavers`
    particles that leave for the block on the other side. `triple` = (stayers, newcomers from the same block, newcomers from another
    block) fixes the members of `cell` — `A` then counts the third entry. `big`: that many more arrivals into a third cell."""
    p = _Placer(dim, TARGETS[dim][cell], _rng("steady", dim, R, A, changers, leavers, cell, triple, arr_cells, big, changers_last))
    bw, t = p.bw, p.t
    new_same = 0 if triple is None else triple[1]
    if triple is not None:
        assert A == triple[2]
    # the generic changers: into a cell of the second x layer, away from every cell the arrivals enter; or into the block's last cell
    if changers_last:
        assert p.sy > 0 and cell == 24
        g_dst = (bw - 1,) * dim
    elif dim == 3:
        g_dst = (1, 2 if p.sy > 0 else 1, 2)
    else:
        g_dst = (1, 5 if p.sy > 0 else 2)
    g_src = p.enter_y(g_dst, changers)
    fixed = {}
    if triple is not None:
        fixed[t] = triple[0]
    cells = [_cell_of_key(k, dim) for k in range(NPB)]
    if changers_last:       # residents only in front of the changers' cell: the changers are the last entries of the previous run
        cells = cells[:_key_of_cell(g_src, dim)]
    n_res = R - changers - leavers - new_same
    for c, n in _spread(n_res, cells, fixed).items():
        p.residents(c, n)
    out_x = bw - 1 if p.sx > 0 else 0
    p.leave_x((out_x, 1 if p.sy > 0 else bw - 2) + ((0,) if dim == 3 else ()), leavers)
    p.enter_y(t, new_same)
    first = A - A // 2 if arr_cells == 2 else A
    p.enter_x(t, first)
    if dim == 3:
        second, third = (t[0], t[1], t[2] ^ 1), (t[0], t[1], (t[2] + 2) % 4)
    else:
        second, third = (t[0], (t[1] + 2) % 8), (t[0], (t[1] + 4) % 8)
    p.enter_x(second, A - first)
    p.enter_x(third, big)
    return _scene(p.positions(), p.velocity)


def source_block(dim, cell=24):
    """the block the arrivals of steady_scene come from"""
    t = TARGETS[dim][cell]
    b = list(target_block(dim))
    b[0] += -1 if t[0] == 0 else 1
    return tuple(b)


def rebuild_scene(dim, R, cell=24, count=None):
    """The first substep of `R` particles in the target block (`count`: exactly that many of them in local cell `cell`)."""
    p = _Placer(dim, TARGETS[dim][cell], _rng("rebuild", dim, R, cell, count))
    fixed = {} if count is None else {p.t: count}
    for c, n in _spread(R, [_cell_of_key(k, dim) for k in range(NPB)], fixed).items():
        p.residents(c, n)
    return _scene(p.positions(), p.velocity)


def touch_scene(dim, nblocks, n=None, order="grouped"):
    """`n` particles (default: one workgroup of launch 1) in the caller's order, every SORT_THREADS of them over exactly `nblocks` distinct
    blocks in a row along x. `order`: "grouped" — block after block, the last block's particles last in their workgroup —, "first" — the
    last block's particles first —, "mixed" — round robin: every wave meets every block."""
    n = SORT_THREADS if n is None else n
    rng = _rng("touch", dim, nblocks, n, order)
    bw = bw_of(dim)
    which = np.arange(SORT_THREADS) % nblocks
    if order != "mixed":
        which = np.sort(which)
        if order == "first":
            which = np.concatenate([which[which == nblocks - 1], which[which != nblocks - 1]])
    which = np.tile(which, n // SORT_THREADS)
    base = np.asarray(target_block(dim), np.float64) * bw + 0.5
    pos = base + rng.integers(0, bw, (n, dim)) + rng.uniform(0.05, 0.70, (n, dim))
    pos[:, 0] += which * bw
    return _scene(pos, (SPEED, SPEED, 0.0)[:dim])


# ------------------------------------------------------------------------------------------------ the case table
# One row per case and dimension. `predicates`: the comparisons of the kernel the row sits on; `build`: (builder, keyword arguments);
# `substeps`: K, or 1 for a rebuild substep; `block`: "target" or "source"; `expect`: the designed value of every block-level field of
# paths(); `cell`: (local cell, {field: value}) of one cell; `wg`: the distinct blocks of every workgroup (TOUCH_SET rows).
Row = collections.namedtuple("Row", "name dim predicates build substeps block expect cell wg last_change")
BLOCK_FIELDS = ("runlen", "narr", "btotal", "dirty", "in_lds", "par", "out_lds", "second_half", "on_lists")
CELL_FIELDS = ("stayed", "new_same", "new_other", "total", "network", "cached", "coop", "select")
ROWS = []


def _add(name, dims, predicates, builder, expect, at=None, substeps=K, block="target", wg=None, last_change=False, **kw):
    assert len(expect) == len(BLOCK_FIELDS)
    for dim in dims:
        ROWS.append(Row(f"{name}-{dim}d", dim, tuple(predicates), (builder, dict(kw, dim=dim)), substeps, block,
                        dict(zip(BLOCK_FIELDS, expect)), at, wg, last_change))


def _cellx(cell, stayed, new_same, new_other, network=False, cached=False, coop=False, select=False):
    return cell, dict(stayed=stayed, new_same=new_same, new_other=new_other, total=stayed + new_same + new_other,
                      network=network, cached=cached, coop=coop, select=select)


T, F = True, False
CH = 3      # in-block changers of a block-level row
#                                                                       runlen      narr btotal        dirty in_lds par out second lists
# ---- in_lds: runlen against RUNCAP
_add("in_lds-below", (3, 2), ["in_lds", "out_lds", "par"], steady_scene, (RUNCAP - 1, 0, RUNCAP - 1, T, T, T, T, T, F), R=RUNCAP - 1)
_add("in_lds-at", (3, 2), ["in_lds", "out_lds", "par"], steady_scene, (RUNCAP, 0, RUNCAP, T, T, T, T, T, F), R=RUNCAP)
_add("in_lds-above", (3, 2), ["in_lds", "out_lds"], steady_scene, (RUNCAP + 1, 0, RUNCAP + 1, T, F, F, F, F, F), R=RUNCAP + 1)
_add("in_lds-above-out-below", (3, 2), ["in_lds", "out_lds"], steady_scene, (RUNCAP + 1, 0, RUNCAP - 1, T, F, F, T, F, F), R=RUNCAP + 1, leavers=2)
# ---- par: runlen + min(narr, BLK_ARR) against RUNCAP; out_lds: btotal against RUNCAP
_add("par-at", (3, 2), ["par", "out_lds"], steady_scene, (RUNCAP - 1, 1, RUNCAP, T, T, T, T, T, F), R=RUNCAP - 1, A=1)
_add("par-above", (3, 2), ["par", "out_lds"], steady_scene, (RUNCAP, 1, RUNCAP + 1, T, T, F, F, T, F), R=RUNCAP, A=1)
_add("par-at-full-array", (3, 2), ["par", "out_lds", "on_lists"], steady_scene, (RUNCAP - BLK_ARR, BLK_ARR, RUNCAP, T, T, T, T, T, F),
     R=RUNCAP - BLK_ARR, A=BLK_ARR)
_add("par-above-full-array", (3, 2), ["par", "out_lds", "on_lists"], steady_scene, (RUNCAP - BLK_ARR + 1, BLK_ARR, RUNCAP + 1, T, T, F, F, T, F),
     R=RUNCAP - BLK_ARR + 1, A=BLK_ARR)
_add("par-sum-at-but-listed", (3, 2), ["par", "out_lds", "on_lists"], steady_scene, (RUNCAP - BLK_ARR - 1, BLK_ARR + 1, RUNCAP, T, T, F, T, T, T),
     R=RUNCAP - BLK_ARR - 1, A=BLK_ARR + 1)
# ---- the block's array of arrivals against the cells' lists: narr against BLK_ARR
for _a, _lists in ((BLK_ARR - 1, F), (BLK_ARR, F), (BLK_ARR + 1, T)):
    for _cells in (1, 2):
        _add(f"array-{_a}-over-{_cells}", (3, 2), ["on_lists"], steady_scene, (300, _a, 300 + _a, T, T, not _lists, T, F, _lists), R=300, A=_a,
             arr_cells=_cells)
# ---- the second staging batch: runlen against 64 (PAR_R / 2); the changers are the last entries of the run
for _r in (HALF - 1, HALF, HALF + 1):
    _add(f"second-batch-{_r}", (3, 2), ["second_half"], steady_scene, (_r, 0, _r, T, T, T, T, _r > HALF, F), R=_r, changers_last=True, last_change=True)
# ---- the last, partly filled round of a staged run
for _r in (1, 63, 64, 65, 128, 129):
    for _a in (0, 1):
        _add(f"tail-{_r}-{_a}", (3, 2), ["tail"], steady_scene, (_r, _a, _r + _a, T, T, T, T, F, F), R=_r, A=_a, changers=min(CH, _r))
# ---- a clean block (no in-block changer) with arrivals only
for _a, _lists in ((1, F), (BLK_ARR, F), (BLK_ARR + 1, T)):
    _add(f"clean-{_a}", (3, 2), ["on_lists"], steady_scene, (300, _a, 300 + _a, F, T, not _lists, T, F, _lists), R=300, A=_a, changers=0)
# ---- a block that everybody leaves while its neighbour receives them: towards +x (nobody's "+" neighbour any more, it goes inactive) and
# towards -x (it stays active, empty, as the receiving block's "+" neighbour)
_add("all-leave-to-plus", (3, 2), ["emptied"], steady_scene, (40, 0, 0, T, T, T, T, F, F), R=300, A=40, block="source")
_add("all-leave-to-minus", (3, 2), ["emptied"], steady_scene, (40, 0, 0, T, T, T, T, F, F), R=300, A=40, cell=63, block="source")
# ---- per cell, wave-parallel form: the newcomers of a cell against NEWC
for _st in (5, 0):
    for _same, _other in ((3, 0), (4, 0), (0, 4), (2, 2), (5, 0), (0, 5), (3, 2)):
        _add(f"newc-{_st}+{_same}+{_other}", (3, 2) if (_same, _other) in ((4, 0), (3, 2)) else (3,), ["NEWC"], steady_scene,
             (200, _other, 200 + _other, T, T, T, T, F, F), _cellx(24, _st, _same, _other, network=_same + _other <= NEWC),
             R=200, A=_other, triple=(_st, _same, _other))
for _cell in (0, 63):
    for _same, _other in ((2, 2), (3, 2)):
        _add(f"newc-cell{_cell}-5+{_same}+{_other}", (3, 2) if _same == 3 else (3,), ["NEWC"], steady_scene, (200, _other, 200 + _other, T, T, T, T, F, F),
             _cellx(_cell, 5, _same, _other, network=_same + _other <= NEWC), R=200, A=_other, triple=(5, _same, _other), cell=_cell)
# ---- per cell, lane-by-lane form (forced by BLK_ARR + 1 more arrivals into another cell, or by runlen + narr > RUNCAP): arrivals against ARRC
BIG = BLK_ARR + 1
for _n in (ARRC - 1, ARRC, ARRC + 1):
    _add(f"arrc-same-{_n}", (3, 2) if _n >= ARRC else (3,), ["ARRC"], steady_scene, (200, BIG, 200 + BIG, T, T, F, T, F, T),
         _cellx(24, 5, _n, 0, cached=_n <= ARRC, coop=_n > ARRC), R=200, triple=(5, _n, 0), big=BIG)
    _add(f"arrc-other-{_n}", (3, 2) if _n >= ARRC else (3,), ["ARRC"], steady_scene, (RUNCAP - 2, _n, RUNCAP - 2 + _n, T, T, F, F, T, F),
         _cellx(24, 5, 0, _n, cached=_n <= ARRC, select=_n > ARRC), R=RUNCAP - 2, A=_n, triple=(5, 0, _n))
# ---- per cell, lane form with more than ARRC arrivals: the cell's total against 64
for _tot in (63, 64, 65):
    for _cell in ((24, 0, 63) if _tot == 64 else (24,)):
        _add(f"coop-{_tot}-cell{_cell}", (3, 2) if _cell == 24 else (3,), ["coop"], steady_scene, (300, 2 + BIG, 300 + 2 + BIG, T, T, F, T, F, T),
             _cellx(_cell, _tot - 5, 3, 2, coop=_tot <= 64, select=_tot > 64), R=300, A=2, triple=(_tot - 5, 3, 2), big=BIG, cell=_cell)
# ---- the rebuild substep: everybody on a list
for _n in (1, ARRC, ARRC + 1, 64, 65):
    _add(f"rebuild-cell-{_n}", (3, 2) if _n in (ARRC + 1, 65) else (3,), ["rebuild"], rebuild_scene, (0, 0, _n + 130, F, T, F, T, F, T),
         _cellx(24, 0, 0, _n, cached=_n <= ARRC, coop=ARRC < _n <= 64, select=_n > 64), substeps=1, R=_n + 130, count=_n)
_add("rebuild-block-at", (3, 2), ["rebuild", "out_lds"], rebuild_scene, (0, 0, RUNCAP, F, T, F, T, F, T), substeps=1, R=RUNCAP)
_add("rebuild-block-above", (3, 2), ["rebuild", "out_lds"], rebuild_scene, (0, 0, RUNCAP + 1, F, T, F, F, F, T), substeps=1, R=RUNCAP + 1)
# ---- launch 1 of a rebuild substep: the distinct blocks of a workgroup against TOUCH_SET
_NONE = (None,) * len(BLOCK_FIELDS)
for _n in (1, 2):
    for _nb in (TOUCH_SET - 1, TOUCH_SET, TOUCH_SET + 1):
        _add(f"touch-{_nb}-x{_n}", (3, 2) if _nb == TOUCH_SET + 1 else (3,), ["TOUCH_SET"], touch_scene, _NONE, substeps=1, block=None, wg=[_nb] * _n,
             nblocks=_nb, n=_n * SORT_THREADS)
    for _order in ("first", "mixed"):
        _add(f"touch-{TOUCH_SET + 1}-{_order}-x{_n}", (3,), ["TOUCH_SET"], touch_scene, _NONE, substeps=1, block=None, wg=[TOUCH_SET + 1] * _n,
             nblocks=TOUCH_SET + 1, n=_n * SORT_THREADS, order=_order)

ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS), "two rows of one name"


def build(row):
    builder, kw = row.build
    return builder(**kw)


def block_of(row):
    if row.block == "source":
        return source_block(row.dim, row.build[1].get("cell", 24))
    return target_block(row.dim)


def check_paths(row, pos_a, pos_b):
    """paths() of the row's block equals the row, field by field (==: a scene that drifted off its boundary says so); returns the facts"""
    f = facts(pos_a, pos_b, row.dim)
    if row.wg is not None:
        got = workgroup_blocks(pos_b, row.dim)
        assert got == row.wg, f"{row.name}: distinct blocks per workgroup {got}, designed {row.wg}"
        return f
    p = paths(f, block_of(row))
    got = {k: getattr(p, k) for k in BLOCK_FIELDS}
    assert got == row.expect, f"{row.name}: the block meets {got}, designed {row.expect}"
    if row.cell is not None:
        key, want = row.cell
        got = {k: (bool if isinstance(want[k], bool) else int)(getattr(p, k)[key]) for k in CELL_FIELDS}
        assert got == want, f"{row.name}: cell {key} meets {got}, designed {want}"
    if row.last_change:
        # the entries of the previous run from index 64 (PAR_R / 2) on — what only the second staging batch brings — change cell
        bw = bw_of(row.dim)
        ca, cb = f["cell_a"], f["cell_b"]
        mine = np.flatnonzero((ca // bw == np.asarray(block_of(row))).all(1))
        run = mine[np.lexsort((mine, local_key(ca[mine], row.dim)))]
        changed = (ca[run] != cb[run]).any(1)
        assert changed[HALF:].all() and changed.sum() == CH, f"{row.name}: the entries behind index {HALF} of the previous run do not all change cell"
        assert changed[-CH:].all(), f"{row.name}: the changers are not the last entries of the previous run"
    return f


# the quantity each threshold predicate compares and its threshold: the coverage test wants the threshold and one to either side, in 3D
THRESHOLDS = {
    "in_lds": (lambda p, c: p.runlen, RUNCAP),
    "par": (lambda p, c: p.runlen + min(p.narr, BLK_ARR), RUNCAP),
    "on_lists": (lambda p, c: p.narr, BLK_ARR),
    "second_half": (lambda p, c: p.runlen, HALF),
    "out_lds": (lambda p, c: p.btotal, RUNCAP),
    "NEWC": (lambda p, c: int(p.new_same[c] + p.new_other[c]) if p.par else None, NEWC),
    "ARRC": (lambda p, c: int(p.new_same[c] + p.new_other[c]) if not p.par else None, ARRC),
    "coop": (lambda p, c: int(p.total[c]) if (not p.par and p.new_same[c] + p.new_other[c] > ARRC) else None, 64),
}
