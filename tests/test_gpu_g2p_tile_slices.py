"""-m gpu: the neo-Hookean one-chunk fused G2P in 3D stages, of its block's node tile, only the z-slices that its chunk's cells reach
(g2p_body.inc, SLICES; the corotated kernel keeps the whole tile and runs the same scenes for the day SLICES is extended). The two-chunk shape (WGS_DEBUG G2P_TWO_PASSES) keeps whole-tile staging and the same arithmetic, so it is the reference: particle
fields, grid and block lists must be the same bits. Every scene runs without colliders (the single-body kernel) and with the floor
cuboid (the main body of the paired launch), under the neo-Hookean and the corotated model."""
import numpy as np
import pytest

from wgsparkl_amd import scenes
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_NEO_HOOKEAN, ElasticCoefficients, ParticlePhase
from wgsparkl_amd.solver import ParticleSet

from helpers import CDF_FIELDS, assert_same_bits, assert_same_grid, debug, step_chunks

pytestmark = pytest.mark.gpu

MODELS = pytest.mark.parametrize("model", [MODEL_NEO_HOOKEAN, MODEL_COROTATED], ids=["neo_hookean", "corotated"])
FLOOR = pytest.mark.parametrize("floor", [False, True], ids=["no_collider", "floor"])


def _cell(pos):
    """the cell a particle is associated with, h = 1"""
    return np.rint(pos).astype(np.int64) - 1


def _scene(pos, floor, model, vel=None):
    """the material, floor and time step of scenes.neo_hookean_cube around the given positions"""
    sc = scenes.neo_hookean_cube(n_side=2, with_floor=floor)
    sc["particles"] = ParticleSet.uniform(pos, 0.25, 2700.0, ElasticCoefficients.from_young_modulus(1.0e7, 0.2),
                                          phase=ParticlePhase(1.0, scenes.FLT_MAX), vel=vel)
    sc["grid_capacity"] = 1024
    sc["model"] = model
    return sc


def _both_shapes_agree(sc, chunks, monkeypatch):
    def run():
        data = step_chunks(sc, chunks)
        st = data.stats()
        assert st["overflow"] == 0, st
        return data.read_particles(), data.read_grid(), data.read_blocks(), st
    a, ga, ka, sa = run()
    with debug(monkeypatch, "G2P_TWO_PASSES"):
        b, gb, kb, _ = run()
    assert np.isfinite(a.pos).all()
    assert_same_bits(a, b, CDF_FIELDS)
    assert_same_grid(ga, gb)
    assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[2], kb[2])   # (block set and counts; where a block sits in memory is up to the atomics)
    return a, sa


@MODELS
@FLOOR
def test_dense_cube_in_free_fall(hip_libs, monkeypatch, floor, model):
    """16^3 particles at 8 per cell, moved so that they fill 2 x 2 x 2 blocks (a particle's cell is rint(x / h) - 1): a chunk is half
    a z-layer of its block and needs three slices; the chunks of cell layer z = 3 need the "+z" rim, slices 3 .. 5."""
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=floor)
    sc["model"] = model
    sc["particles"].pos[:] += np.float32(0.35)
    assert len(np.unique(_cell(sc["particles"].pos) // 4, axis=0)) == 8 and len(np.unique(_cell(sc["particles"].pos), axis=0)) == 512
    _both_shapes_agree(sc, (1, 9), monkeypatch)


@MODELS
@FLOOR
def test_sparse_lattice_needs_every_slice(hip_libs, monkeypatch, floor, model):
    """One particle per cell over 3 x 3 x 3 blocks: a chunk of 64 spans a whole block, all four cell layers, all six slices."""
    pos = scenes.lattice((12, 12, 12), (20.5, 8.5, 20.5), 2.0, jitter=0.1, seed=5)   # (spacing 1 = h: lattice() places at half its cell width)
    assert len(np.unique(_cell(pos), axis=0)) == 12 ** 3 and len(np.unique(_cell(pos) // 4, axis=0)) == 27
    _both_shapes_agree(_scene(pos, floor, model), (1, 9), monkeypatch)


@MODELS
@FLOOR
def test_ragged_cells_moving_across_cells_and_blocks(hip_libs, monkeypatch, floor, model):
    """2 .. 12 particles per cell (seeded) in a box that starts and ends inside blocks, moving half a cell per substep along the
    diagonal, away from the floor, for 20 substeps: chunks straddle z-layers and blocks, the last chunk is partial, particles change
    cell and block every few substeps, so the sort rebuilds the runs the ranges are taken from."""
    rng = np.random.default_rng(17)
    cells = np.stack(np.meshgrid(np.arange(21, 31), np.arange(9, 18), np.arange(22, 33), indexing="ij"), -1).reshape(-1, 3)
    per_cell = rng.integers(2, 13, len(cells))
    pos = (np.repeat(cells, per_cell, axis=0) + 1.0 + rng.uniform(-0.45, 0.45, (int(per_cell.sum()), 3))).astype(np.float32)
    pos = pos[rng.permutation(len(pos))]
    assert len(pos) % 64 != 0 and np.array_equal(np.unique(_cell(pos), axis=0, return_counts=True)[1], per_cell)
    dt = scenes.neo_hookean_cube(n_side=2)["params"].dt
    vel = np.full(pos.shape, 0.5 / dt / np.sqrt(3.0), np.float32)
    a, st = _both_shapes_agree(_scene(pos, floor, model, vel=vel), (1, 7, 12), monkeypatch)
    assert st["cell_changers"] > 0
    assert (_cell(a.pos) // 4 != _cell(pos) // 4).any(axis=1).mean() > 0.5   # most particles ended in another block


@MODELS
def test_landed_cube_takes_its_range_from_the_unlisted_lanes(hip_libs, monkeypatch, model):
    """The cube lowered onto the floor, shifted by half a block so that chunks hold particles of listed (near-collider) and of
    unlisted blocks: the main body of the paired launch advances the unlisted lanes only, and the slices come from their cells."""
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=True)
    sc["model"] = model
    sc["particles"].pos[:, 1] -= 5.6
    sc["particles"].pos[:, 0] += 1.5
    sc["particles"].vel[:, 0] = 1.5
    _, st = _both_shapes_agree(sc, (1, 19), monkeypatch)
    assert 0 < st["num_near_collider_blocks"] < st["num_active_blocks"], st
