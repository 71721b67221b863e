"""The quad table of wgsparkl_amd/sharded.py is the one of csrc/layout.h: `static constexpr int NAME = k;` of Pl<3> and Pl<2>,
name for name and number for number, and an exchange record is NQ quads and two words, as kernels_shard.h states it."""
import os
import re

import pytest

from wgsparkl_amd.sharded import QUADS, record_floats

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wgsparkl_amd", "csrc")


def _read(name):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def _pl(dim):
    """the constants of `template <> struct Pl<dim> { ... };` in the order of the header"""
    body = re.search(r"template <> struct Pl<%d> \{(.*?)\n\};" % dim, _read("layout.h"), re.S)
    assert body, f"layout.h has no Pl<{dim}>"
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*static constexpr int (\w+) = (\d+);", body.group(1), re.M)}


@pytest.mark.parametrize("dim", [3, 2])
def test_python_quad_table_is_layout_h(dim):
    header = _pl(dim)
    assert header["NQ"] == max(header.values()) > 0          # (the parse found the table, and NQ closes it)
    assert QUADS[dim] == header
    assert list(QUADS[dim]) == list(header), "same order as the header, so that the two read side by side"


@pytest.mark.parametrize("dim", [3, 2])
def test_record_is_nq_quads_and_two_words(dim):
    stated = re.search(r"template <int D> constexpr int particle_record_floats\(\) \{ return Pl<D>::NQ \* (\d+) \+ (\d+); \}",
                       _read("kernels_shard.h"))
    assert stated, "kernels_shard.h no longer states particle_record_floats as NQ * a + b"
    assert (int(stated.group(1)), int(stated.group(2))) == (4, 2)
    assert record_floats(dim) == _pl(dim)["NQ"] * 4 + 2
