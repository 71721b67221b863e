"""No GPU: what MpmData.from_scene and NativeShard.from_scene make of a scene dict (the key table in the docstring of
wgsparkl_amd/scenes.py) — the creation and the setters they call, in order, with the constructors replaced by recorders."""
import numpy as np
import pytest

from wgsparkl_amd import MpmData
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_FLUID, MODEL_NEO_HOOKEAN, Wall
from wgsparkl_amd.sharded import INT_MAX, INT_MIN, NativeShard, SlabPartition

REQUIRED = dict(params="params", particles="particles", colliders=["c"], cell_width=0.5, grid_capacity=64)
TABLE = np.array([2, 2, 1], np.uint8)
WALLS = [Wall(1, 0.0, 3), None, None, None]
OPTIONAL = dict(model=MODEL_NEO_HOOKEAN, fluid_gamma=5.0, models=TABLE, walls=WALLS)


@pytest.fixture
def calls(monkeypatch):
    """the calls MpmData.from_scene makes, in order: ("new", the seven arguments) and (setter name, its argument)"""
    log = []

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("set_"):
                raise AttributeError(name)
            return lambda value: log.append((name, value))

    def new(cls, *args):
        log.append(("new", args))
        return Recorder()

    monkeypatch.setattr(MpmData, "new", classmethod(new))
    return log


def _create(model):
    return ("new", ("pipe", "params", "particles", ["c"], 0.5, 64, model))


def test_every_optional_key_is_applied_in_order(calls):
    MpmData.from_scene("pipe", {**REQUIRED, **OPTIONAL, "solid_model": 1, "fluid": "ignored"})
    assert calls == [_create(MODEL_NEO_HOOKEAN), ("set_fluid_eos", 5.0), ("set_particle_models", TABLE), ("set_domain_walls", WALLS)]


def test_a_scene_without_the_keys_is_created_and_nothing_else(calls):
    MpmData.from_scene("pipe", REQUIRED)
    assert calls == [_create(MODEL_COROTATED)]
    del calls[:]
    MpmData.from_scene("pipe", {**REQUIRED, "fluid_gamma": None, "models": None, "walls": None})
    assert calls == [_create(MODEL_COROTATED)]


@pytest.mark.parametrize("key,setter", [("fluid_gamma", "set_fluid_eos"), ("models", "set_particle_models"), ("walls", "set_domain_walls")])
def test_none_as_an_override_drops_exactly_its_own_call(calls, key, setter):
    MpmData.from_scene("pipe", {**REQUIRED, **OPTIONAL}, **{key: None})
    assert [c[0] for c in calls] == [n for n in ("new", "set_fluid_eos", "set_particle_models", "set_domain_walls") if n != setter]
    assert calls[0] == _create(MODEL_NEO_HOOKEAN)


def test_a_value_override_replaces_the_scenes_entry(calls):
    other = np.zeros(3, np.uint8)
    MpmData.from_scene("pipe", {**REQUIRED, **OPTIONAL}, model=MODEL_FLUID, fluid_gamma=3.0, models=other, cell_width=0.25, colliders=[])
    assert calls == [("new", ("pipe", "params", "particles", [], 0.25, 64, MODEL_FLUID)), ("set_fluid_eos", 3.0), ("set_particle_models", other),
                     ("set_domain_walls", WALLS)]


# ------------------------------------------------------------------------------------------------ slabs
SLAB = dict(REQUIRED, model=MODEL_FLUID, global_ids="ids", partition=SlabPartition([2, 5, 9, 12]), uniform_material=(1.0, 2.0, 3.0, 4.0))


@pytest.fixture
def shard_calls(monkeypatch):
    """the constructor calls of NativeShard (positional arguments behind the pipeline, keywords) and its set_fluid_eos calls"""
    log = []
    monkeypatch.setattr(NativeShard, "__init__", lambda self, pipeline, *args, **kw: log.append(("init", args, kw)))
    monkeypatch.setattr(NativeShard, "set_fluid_eos", lambda self, gamma: log.append(("set_fluid_eos", gamma)))
    monkeypatch.setattr(NativeShard, "__del__", lambda self: None)
    return log


@pytest.mark.parametrize("rank,lo,hi,lower,upper", [(0, INT_MIN, 5, False, True), (1, 5, 9, True, True), (2, 9, INT_MAX, True, False)])
def test_a_slab_takes_its_range_and_neighbours_from_the_partition(shard_calls, rank, lo, hi, lower, upper):
    NativeShard.from_scene("pipe", SLAB, rank, "comm", particle_capacity=100, migrant_capacity=7)
    (_, args, kw), = shard_calls
    assert args == ("params", "particles", "ids", ["c"], 0.5, 64, lo, hi, lower, upper, 100)
    assert kw == dict(model=MODEL_FLUID, force_plastic=False, halo_capacity_records=4096, migrant_capacity=7, comm="comm",
                      uniform_material=(1.0, 2.0, 3.0, 4.0))


def test_a_slab_gets_the_exponent_and_the_defaults(shard_calls):
    scene = {k: v for k, v in SLAB.items() if k not in ("model", "uniform_material")}
    NativeShard.from_scene("pipe", {**scene, "fluid_gamma": 5.0}, 0, force_plastic=True)
    (_, args, kw), eos = shard_calls
    assert args[-1] == 0 and kw == dict(model=MODEL_COROTATED, force_plastic=True, halo_capacity_records=4096, migrant_capacity=4096, comm=None,
                                        uniform_material=None)
    assert eos == ("set_fluid_eos", 5.0)
    del shard_calls[:]
    NativeShard.from_scene("pipe", {**scene, "fluid_gamma": 5.0}, 0, fluid_gamma=None)
    assert [c[0] for c in shard_calls] == ["init"]


@pytest.mark.parametrize("key,value", [("models", TABLE), ("walls", WALLS)])
def test_a_slab_refuses_single_domain_keys_unless_overridden(shard_calls, key, value):
    with pytest.raises(ValueError, match=key):
        NativeShard.from_scene("pipe", {**SLAB, key: value}, 1)
    assert not shard_calls
    NativeShard.from_scene("pipe", {**SLAB, key: value}, 1, **{key: None})
    NativeShard.from_scene("pipe", {**SLAB, key: None}, 1)
    assert [c[0] for c in shard_calls] == ["init", "init"]
