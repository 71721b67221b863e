"""bench.py --dump-outputs: the particle state of a leg as float32 .npy files, the same for the same inputs, within the
size budget (a seeded sample of the rows above it). The device read-back is stood in for by the scene's own particles."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from wgsparkl_amd import scenes  # noqa: E402


class _Data:
    def __init__(self, scene):
        self.scene = scene

    def read_particles(self):
        return self.scene["particles"]

    def read_body_poses(self):
        return [dict(rotation=np.array([0.0, 0.0, 0.0, 1.0]), translation=np.array(c.translation, np.float64),
                     linvel=np.zeros(3), angvel=np.zeros(3), com=np.zeros(3)) for c in self.scene["colliders"]]


class _Leg:
    sharded = False

    def __init__(self, scene):
        self.scene = scene
        self.data = _Data(scene)


def _dump(scene, path):
    bench.dump_outputs(_Leg(scene), str(path), 0, 1)
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_writes_every_particle_field_in_float32(tmp_path):
    sc = scenes.neo_hookean_cube(n_side=8, with_floor=True)
    out = _dump(sc, tmp_path)
    assert sorted(out) == ["affine", "bodies", "def_grad", "pos", "vel"]
    assert all(a.dtype == np.float32 for a in out.values())
    ps = sc["particles"]
    for k in ("pos", "vel", "def_grad", "affine"):
        assert np.array_equal(out[k], getattr(ps, k))
    assert out["bodies"].shape == (1, 13)


def test_dump_of_a_plastic_scene_holds_the_plastic_state(tmp_path):
    sc = scenes.sand_column(nx=8, ny=8, nz=8)
    out = _dump(sc, tmp_path)
    assert np.array_equal(out["plastic_state"], sc["particles"].dp_state)
    assert "bodies" not in out


def test_dump_above_the_budget_is_the_same_seeded_sample_every_time(tmp_path, monkeypatch):
    sc = scenes.neo_hookean_cube(n_side=10)
    row_bytes = (3 + 3 + 9 + 9) * 4
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100 * row_bytes)
    a = _dump(sc, tmp_path / "a")
    b = _dump(sc, tmp_path / "b")
    assert all(len(v) == 100 for v in a.values())
    for k in a:
        assert np.array_equal(a[k], b[k])
    pos = sc["particles"].pos
    rows = [int(np.flatnonzero((pos == p).all(1))[0]) for p in a["pos"]]
    assert rows == sorted(rows)                     # a subset of the rows, in their order
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 100 * row_bytes + 4096


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse_args()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.full and a.dump_outputs == "d"
