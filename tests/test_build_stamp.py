"""-m "not gpu": csrc/build.sh decides "up to date" by content, not by file time. Beside each library sits <lib>.stamp, a
sha256 over the sources, the dimension and the flag line (and the library's own sha256): a library that was put there by
hand, or built with other WGS_EXTRA_FLAGS, is rebuilt; a source that was only touched is not. Works on a copy of csrc/ and
include/ with $HIPCC pointing at a stub that logs its call and writes a small file, so no compile is paid."""
import os
import shutil
import stat
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = """#!/bin/bash
echo "$@" >> "$STUB_LOG"
while [[ $# -gt 1 ]]; do
  if [[ "$1" == "-o" ]]; then echo "stub library for: $STUB_TAG" > "$2"; fi
  shift
done
"""


class Tree:
    def __init__(self, tmp_path):
        self.csrc = tmp_path / "wgsparkl_amd" / "csrc"
        shutil.copytree(os.path.join(ROOT, "wgsparkl_amd", "csrc"), self.csrc, ignore=shutil.ignore_patterns("*.so*"))
        shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
        self.log = tmp_path / "hipcc_calls.log"
        self.hipcc = tmp_path / "hipcc_stub.sh"
        self.hipcc.write_text(STUB)
        self.hipcc.chmod(self.hipcc.stat().st_mode | stat.S_IXUSR)
        self.libs = [self.csrc / f"libwgsparkl{dim}d_hip.so" for dim in (2, 3)]

    def build(self, *args, flags=None, out_dir=None):
        """Runs build.sh; returns how many times it called the compiler."""
        env = {k: v for k, v in os.environ.items() if k not in ("WGS_EXTRA_FLAGS", "WGS_OUT_DIR", "WGS_ARCH")}
        env.update(HIPCC=str(self.hipcc), STUB_LOG=str(self.log), STUB_TAG=flags or "plain")
        if flags is not None:
            env["WGS_EXTRA_FLAGS"] = flags
        if out_dir is not None:
            env["WGS_OUT_DIR"] = str(out_dir)
        self.log.write_text("")
        subprocess.run(["bash", str(self.csrc / "build.sh"), *args], env=env, check=True, timeout=60)
        return len(self.log.read_text().splitlines())


@pytest.fixture
def tree(tmp_path):
    t = Tree(tmp_path)
    assert t.build() == 2           # nothing there: one compile per dimension
    assert all(p.exists() and os.path.exists(f"{p}.stamp") for p in t.libs)
    return t


def test_a_second_build_compiles_nothing(tree):
    assert tree.build() == 0


def test_a_replaced_library_with_a_newer_time_is_rebuilt(tree):
    lib = tree.libs[1]
    lib.write_text("a variant copied over the library")
    later = os.stat(tree.csrc / "capi.hip").st_mtime + 1000
    os.utime(lib, (later, later))    # the newest file of the directory: what the file-time rule took for current
    assert tree.build() == 1
    assert lib.read_text().startswith("stub library")
    assert tree.build() == 0


def test_other_extra_flags_are_rebuilt(tree):
    assert tree.build(flags="-DWGS_ABLATE") == 2
    assert tree.build(flags="-DWGS_ABLATE") == 0
    assert tree.build() == 2        # and a plain build does not take the ablated libraries for current


def test_a_touched_source_with_the_same_bytes_compiles_nothing(tree):
    later = max(os.stat(p).st_mtime for p in tree.libs) + 1000
    for name in ("capi.hip", "layout.h"):
        os.utime(tree.csrc / name, (later, later))
    assert tree.build() == 0


def test_a_changed_source_is_rebuilt(tree):
    with open(tree.csrc / "layout.h", "a") as f:
        f.write("// one more line\n")
    assert tree.build() == 2


def test_force_always_compiles(tree):
    assert tree.build("force") == 2
    assert tree.build("force") == 2


def test_out_dir_takes_both_libraries_and_leaves_the_ones_beside_the_sources_alone(tree, tmp_path):
    before = [(p.read_bytes(), os.stat(p).st_mtime_ns) for p in tree.libs]
    out = tmp_path / "variants" / "v1"
    assert tree.build(flags="-DV1", out_dir=out) == 2
    assert sorted(os.listdir(out)) == sorted(f"libwgsparkl{d}d_hip.so{s}" for d in (2, 3) for s in ("", ".stamp"))
    assert tree.build(flags="-DV1", out_dir=out) == 0
    assert [(p.read_bytes(), os.stat(p).st_mtime_ns) for p in tree.libs] == before
