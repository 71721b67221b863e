"""-m "not gpu": the step engine of tools/gpu.py, the developer tools' one runner. Every step is a fresh child under
`timeout -k 10 <seconds>`; the chain ends at the first step that fails - by exit status, or by a HIP fault text in its
output even when the status is 0 - names that step and its class, and starts nothing after it. A library variant is chosen
through WGS_LIB_DIR; nothing under tools/ writes to the in-tree libraries. The steps here are tiny Python children that
exit with the numbers; no signal is raised and nothing touches a GPU."""
import importlib.util
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
TREE_LIBS = [os.path.join(ROOT, "wgsparkl_amd", "csrc", f"libwgsparkl{dim}d_hip.so") for dim in (2, 3)]


@pytest.fixture(scope="module")
def gpu():
    spec = importlib.util.spec_from_file_location("tools_gpu", os.path.join(TOOLS, "gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classification_of_exit_statuses(gpu):
    assert {s: gpu.classify(s) for s in (0, 1, 3, 124, 137, 134, -6, 139, -11)} == {
        0: "ok", 1: "failure", 3: "failure", 124: "time limit", 137: "time limit", 134: "abort", -6: "abort",
        139: "segmentation fault", -11: "segmentation fault"}


SECOND_STEPS = {      # what step two does, its time limit -> the class the runner must name
    "exit 139": ("import sys; sys.exit(139)", 20, "segmentation fault"),
    "exit 134": ("import sys; sys.exit(134)", 20, "abort"),
    "over its limit": ("import time; time.sleep(5)", 1, "time limit"),
    "fault text, exit 0": ("print('HIP error: an illegal memory access was encountered')", 20, "fault text"),
    "other fault text, exit 0": ("import sys; print('Memory access fault by GPU node-1', file=sys.stderr)", 20, "fault text"),
    "exit 1": ("import sys; sys.exit(1)", 20, "failure"),
}


@pytest.mark.parametrize("case", list(SECOND_STEPS))
def test_the_chain_ends_at_the_first_step_that_goes_wrong(gpu, tmp_path, capsys, case):
    code, limit, cls = SECOND_STEPS[case]
    marks = [tmp_path / f"ran{i}" for i in (1, 2, 3)]
    touch = "open({!r}, 'w').close(); "
    steps = [gpu.Step("one", [sys.executable, "-c", touch.format(str(marks[0]))], 20, str(tmp_path / "1.log")),
             gpu.Step("two", [sys.executable, "-c", touch.format(str(marks[1])) + code], limit, str(tmp_path / "2.log")),
             gpu.Step("three", [sys.executable, "-c", touch.format(str(marks[2]))], 20, str(tmp_path / "3.log"))]
    status = gpu.run_chain(steps)
    said = capsys.readouterr().err
    assert status != 0
    assert marks[0].exists() and marks[1].exists() and not marks[2].exists()
    assert "step 2 of 3 [two]" in said and cls in said, said
    assert not os.path.exists(tmp_path / "3.log")


def test_a_clean_chain_runs_every_step_in_its_own_environment_and_returns_zero(gpu, tmp_path, capsys):
    code = "import os; print(os.environ.get('WGS_LIB_DIR'))"
    steps = [gpu.Step(f"s{i}", [sys.executable, "-c", code], 20, str(tmp_path / f"{i}.log"), {"WGS_LIB_DIR": f"/variants/{i}"}) for i in (1, 2)]
    seen = []
    steps[1].then = lambda step: seen.append(open(step.log).read().strip())
    assert gpu.run_chain(steps) == 0
    assert seen == ["/variants/2"] and open(tmp_path / "1.log").read().strip() == "/variants/1"
    assert capsys.readouterr().err == ""


def test_dry_run_of_an_ab_plan_prints_every_step_and_touches_nothing(gpu, tmp_path, capsys):
    dirs = {"base": tmp_path / "base", "try1": tmp_path / "try1"}
    for d in dirs.values():
        d.mkdir()
    before = [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in TREE_LIBS if os.path.exists(p)]
    out_dir = tmp_path / "out"
    argv = ["ab", "--dry-run", "--out", str(out_dir), "--cfg", "c2", "c3", "--reps", "2"] + [x for n, d in dirs.items() for x in ("--lib", f"{n}={d}")] + ["--lib", "tree"]
    assert gpu.main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.split("\n") if ln.strip()]
    assert len(lines) == 2 * 3 * 2                       # repetitions x libraries x configurations
    lib_dirs = []
    for ln in lines:
        m = re.match(r"^WGS_LIB_DIR=(\S+) timeout -k 10 \d+ \S*python\S* bench\.py .*--config (c2|c3)\b.* > \S+\.log 2>&1( &&)?$", ln)
        assert m, ln
        assert not re.search(r"\b(cp|mv)\b", ln), ln
        lib_dirs.append((m.group(1), m.group(2)))
    one_rep = [(str(d), cfg) for d in (*dirs.values(), gpu.TREE_LIBS) for cfg in ("c2", "c3")]   # library, then configuration
    assert lib_dirs == one_rep * 2
    assert not out_dir.exists()
    assert [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in TREE_LIBS if os.path.exists(p)] == before


@pytest.mark.parametrize("argv", [["kstats", "c3"], ["kstats", "sand3"], ["kstats", "native", "--", "c5"], ["pmc", "c2", "--set", "fetch", "sq1"],
                                  ["pmc", "stirred"], ["ab", "--legs"], ["ab", "--debug", "262144", "--cfg", "c2"], ["tests", "-k", "shard"]], ids=" ".join)
def test_every_subcommand_plans_steps_under_timeout_with_the_program_after_the_profilers_dashes(gpu, capsys, argv):
    assert gpu.main([argv[0], "--dry-run"] + argv[1:]) == 0
    lines = [ln for ln in capsys.readouterr().out.split("\n") if ln.strip()]
    assert lines
    for ln in lines:
        assert re.match(r"^(\w+=\S+ )*timeout -k 10 \d+ ", ln), ln
        if "rocprofv3" in ln:
            assert re.search(r" rocprofv3 --kernel-trace (--stats|--pmc( [A-Z_0-9]+)+) --output-format csv -d \S+ -- \S*python", ln), ln
    if argv[0] == "pmc":     # a run per counter set
        assert len(lines) == len(argv[3:] if "--set" in argv else ["fetch", "write", "sq1", "sq2"])


WRITES_THE_TREE_LIBRARY = re.compile(r"\b(cp|mv)\b.*csrc/lib|>.*csrc/lib|open\(.*csrc.*[\"']wb?[\"']|(copy|copyfile|copy2|move)\(.*(TREE|csrc)")


def test_no_tool_writes_the_in_tree_libraries():
    assert WRITES_THE_TREE_LIBRARY.search("cp $f wgsparkl_amd/csrc/libwgsparkl3d_hip.so")          # what the old scripts did
    assert WRITES_THE_TREE_LIBRARY.search('subprocess.run(["cp", lib, TREE]); open(csrc_lib, "wb")')
    found = []
    for d, _, files in os.walk(TOOLS):
        if os.path.relpath(d, TOOLS).split(os.sep)[0] == "tmp_libs":
            continue
        for name in files:
            if name.endswith((".py", ".sh", ".hip", ".md")):
                for i, ln in enumerate(open(os.path.join(d, name), errors="replace"), 1):
                    if WRITES_THE_TREE_LIBRARY.search(ln) or re.search(r"[\"']cp[\"'].*TREE", ln):
                        found.append(f"{name}:{i}: {ln.strip()}")
    assert found == []
