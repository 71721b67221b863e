"""The comparers, the WGS_DEBUG block and the restart colliders of tests/helpers.py, on stand-in objects: what the -m gpu tests lean on must
itself fail when it should. No GPU."""
import math
import os
import re
import types

import numpy as np
import pytest

import helpers
from helpers import (BASE_FIELDS, assert_same_bits, assert_same_bodies, assert_same_grid, debug, debug_switches, restored_colliders)
from wgsparkl_amd.solver import Collider


def _particles(**changes):
    p = types.SimpleNamespace(**{f: np.arange(6, dtype=np.float32).reshape(3, 2) + k for k, f in enumerate(BASE_FIELDS)})
    for f, (index, value) in changes.items():
        getattr(p, f)[index] = value
    return p


def test_same_bits_passes_on_equal_fields_and_names_the_field_that_differs():
    assert_same_bits(_particles(), _particles(), BASE_FIELDS)
    with pytest.raises(AssertionError) as e:
        assert_same_bits(_particles(), _particles(def_grad=((1, 0), 7.5)), BASE_FIELDS, "NO_UNIFORM")
    assert "def_grad" in str(e.value) and "NO_UNIFORM" in str(e.value)
    assert_same_bits(_particles(), _particles(def_grad=((1, 0), 7.5)), ("pos", "vel", "affine"))      # only the fields asked for


def test_same_bits_is_array_equal_a_nan_differs_from_itself_and_the_zeros_are_equal():
    with pytest.raises(AssertionError) as e:
        assert_same_bits(_particles(vel=((0, 1), np.nan)), _particles(vel=((0, 1), np.nan)), BASE_FIELDS)
    assert "vel" in str(e.value)
    assert_same_bits(_particles(pos=((0, 0), 0.0)), _particles(pos=((0, 0), -0.0)), BASE_FIELDS)


def test_same_grid_fails_on_another_length_and_on_one_entry():
    grid = lambda: (np.arange(6).reshape(3, 2), np.ones((3, 3), np.float32), np.zeros(3, np.float32))
    assert_same_grid(grid(), grid())
    with pytest.raises(AssertionError):
        assert_same_grid(grid(), grid()[:2])
    other = grid()
    other[1][2, 1] = 2.0
    with pytest.raises(AssertionError):
        assert_same_grid(grid(), other)


def test_same_bodies_fails_on_another_length_and_on_one_entry():
    bodies = lambda: [dict(translation=np.array([1.0, 2.0, 3.0]), linvel=np.zeros(3)), dict(translation=np.zeros(3), linvel=[0.5, 0.0, 0.0])]
    assert_same_bodies(bodies(), bodies())
    with pytest.raises(AssertionError):
        assert_same_bodies(bodies(), bodies()[:1])
    other = bodies()
    other[1]["linvel"] = [0.5, 0.0, 1e-9]
    with pytest.raises(AssertionError) as e:
        assert_same_bodies(bodies(), other)
    assert "linvel" in str(e.value)
    assert_same_bodies(bodies(), other, ("translation",))       # only the keys asked for


@pytest.mark.parametrize("before", [None, "4"])
def test_debug_block_sets_the_switches_and_restores_what_was_there(monkeypatch, before):
    if before is None:
        monkeypatch.delenv("WGS_DEBUG", raising=False)
    else:
        monkeypatch.setenv("WGS_DEBUG", before)
    with debug(monkeypatch, "NO_UNIFORM"):
        assert os.environ["WGS_DEBUG"] == debug_switches("NO_UNIFORM")
        with debug(monkeypatch, "REBIN_LAUNCH", "NO_REBIN"):                      # nested blocks restore in order
            assert os.environ["WGS_DEBUG"] == debug_switches("REBIN_LAUNCH", "NO_REBIN")
        assert os.environ["WGS_DEBUG"] == debug_switches("NO_UNIFORM")
    assert os.environ.get("WGS_DEBUG") == before
    with pytest.raises(ZeroDivisionError):
        with debug(monkeypatch, "NO_UNIFORM"):
            assert os.environ["WGS_DEBUG"] == debug_switches("NO_UNIFORM")
            1 / 0
    assert os.environ.get("WGS_DEBUG") == before


def test_debug_switches_finds_every_switch_of_layout_h():
    a, b = int(debug_switches("NO_UNIFORM")), int(debug_switches("REBIN_LAUNCH"))
    assert a != b and a & (a - 1) == 0 and b & (b - 1) == 0
    assert int(debug_switches("NO_UNIFORM", "REBIN_LAUNCH")) == a | b and debug_switches() == "0"
    with pytest.raises(KeyError):
        debug_switches("NO_SUCH_SWITCH")
    with open(helpers._LAYOUT_H) as f:
        declared = set(re.findall(r"\bDBG_(\w+)\s*=(?!=)", f.read()))
    assert len(declared) >= 20 and set(helpers._debug_bits()) == declared
    assert helpers._debug_bits() is helpers._debug_bits()       # parsed once


def test_restored_colliders_take_over_the_pose_read_back():
    cols = [Collider.cuboid((50.0, 1.0, 50.0), (8.0, 1.0, 8.0)), Collider.ball(1.5, (8.0, 12.0, 8.0), linvel=(0.0, -1.0, 0.0), angvel=(0.0, 0.0, 0.5))]
    q = np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9])
    bodies = [dict(rotation=np.array([0.0, 0.0, 0.0, 1.0]), translation=np.array([8.0, 1.0, 8.0]), linvel=np.zeros(3), angvel=np.zeros(3),
                   com=np.array([8.0, 1.0, 8.0])),
              dict(rotation=q, translation=np.array([8.25, 11.5, 7.75]), linvel=np.array([0.125, -1.5, 0.0]), angvel=np.array([0.0, 0.25, 0.5]),
                   com=np.array([8.25, 11.5, 8.0]))]
    got = restored_colliders(cols, bodies, 3)
    assert len(got) == 2
    for c, c0, b in zip(got, cols, bodies):
        for key in ("rotation", "translation", "linvel", "angvel", "com"):
            assert getattr(c, key) == tuple(b[key]), key
        assert c.shape_type == c0.shape_type and c.shape == c0.shape and c.inv_mass == c0.inv_mass


def test_restored_colliders_hand_a_2d_pose_over_as_an_angle():
    t = 2.5
    col = Collider.cuboid((3.0, 1.0), (5.0, 2.0), rotation=(0.0,))
    body = dict(rotation=np.array([math.cos(t), math.sin(t)]), translation=np.array([5.5, 2.25]), linvel=np.array([0.5, -0.25]),
                angvel=np.array([0.75]), com=np.array([5.5, 2.25]))
    got, = restored_colliders([col], [body], 2)
    assert len(got.rotation) == 1 and abs(got.rotation[0] - t) <= 1e-12
    assert got.linvel == (0.5, -0.25, 0.0) and got.translation == (5.5, 2.25) and got.angvel == (0.75,) and got.com == (5.5, 2.25)
