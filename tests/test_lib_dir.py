"""-m "not gpu": WGS_LIB_DIR (wgsparkl_amd/_ffi.py) chooses the directory both libraries are loaded from - a library variant
is picked by path, never by copying it over the in-tree libraries - and says so on stderr; a file missing there is the
usual ImportError with that path, not a build; unset, every path is the in-tree one. Each case is a fresh child process
(the override is read once per process). No compute call is made here."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgsparkl_amd", "csrc")
NAMES = ("libwgsparkl2d_hip.so", "libwgsparkl3d_hip.so")
CHILD = ("from wgsparkl_amd import _ffi\n"
         "for dim in (2, 3):\n"
         "    lib, _ = _ffi.load(dim)\n"
         "    print(dim, lib.wgs_dim(), lib._name)\n")


def child(lib_dir):
    env = {k: v for k, v in os.environ.items() if k != "WGS_LIB_DIR"}
    if lib_dir is not None:
        env["WGS_LIB_DIR"] = lib_dir
    return subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def test_both_libraries_load_from_the_override_directory(hip_libs, tmp_path):
    for name in NAMES:
        shutil.copy(os.path.join(CSRC, name), tmp_path / name)
    r = child(str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:2] == [f"{dim} {dim} {tmp_path / f'libwgsparkl{dim}d_hip.so'}" for dim in (2, 3)]
    said = [ln for ln in r.stderr.split("\n") if "WGS_LIB_DIR" in ln]
    assert said and all(str(tmp_path) in ln for ln in said), r.stderr


def test_a_missing_library_in_the_override_directory_is_an_import_error_and_builds_nothing(hip_libs, tmp_path):
    before = {name: os.stat(os.path.join(CSRC, name)).st_mtime_ns for name in NAMES}
    r = child(str(tmp_path))
    assert r.returncode != 0
    assert "ImportError" in r.stderr and str(tmp_path / NAMES[0]) in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []
    assert {name: os.stat(os.path.join(CSRC, name)).st_mtime_ns for name in NAMES} == before


def test_unset_the_paths_are_the_in_tree_ones(hip_libs):
    r = child(None)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:2] == [f"{dim} {dim} {os.path.join(CSRC, f'libwgsparkl{dim}d_hip.so')}" for dim in (2, 3)]
    assert "WGS_LIB_DIR" not in r.stderr
    if not os.environ.get("WGS_LIB_DIR"):    # this process too
        assert [hip_libs.lib_path(dim) for dim in (2, 3)] == [os.path.join(CSRC, f"libwgsparkl{dim}d_hip.so") for dim in (2, 3)]
