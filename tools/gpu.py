#!/usr/bin/env python3
"""The one runner of the developer measurements on a GPU machine (standard library only; tools/README.md has the table).

    python tools/gpu.py ab --lib base=tools/tmp_libs/base --lib tree --cfg c2 c3 --reps 3
    python tools/gpu.py kstats c3            python tools/gpu.py pmc sand3 --set fetch write
    python tools/gpu.py tests -k shard       python tools/gpu.py ab --dry-run --lib tree --legs

Every subcommand is a list of steps handed to ONE engine (run_chain): each step is a fresh child process under
`timeout -k 10 <seconds>` with its own environment and log file, and the chain ends at the first step that fails or whose
output holds a HIP fault text - nothing is started on a card after something went wrong on it. A library variant is
chosen by WGS_LIB_DIR (wgsparkl_amd/_ffi.py) in the step's environment; nothing here writes to wgsparkl_amd/csrc.
`--dry-run` prints the plan as shell lines and runs nothing."""
import argparse
import collections
import csv
import glob
import json
import os
import shlex
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIBS = os.path.join(ROOT, "wgsparkl_amd", "csrc")
PY = sys.executable or "python3"

# ---------------------------------------------------------------------------------------------------------- the engine

FAULT_TEXTS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION", "HW Exception by GPU node")


class Step:
    """One child process: argv under a time limit, `env` on top of the runner's environment, stdout and stderr into `log`.
    `then(step)` runs in the runner after the step ended well (a summariser: it reads the log, prints, starts nothing)."""

    def __init__(self, name, argv, limit, log, env=None, then=None):
        self.name, self.argv, self.limit, self.log, self.env, self.then = name, list(argv), int(limit), log, dict(env or {}), then

    def command(self):
        return ["timeout", "-k", "10", str(self.limit)] + self.argv

    def shell_line(self):
        env = "".join(f"{k}={shlex.quote(v)} " for k, v in self.env.items())
        return f"{env}{' '.join(shlex.quote(a) for a in self.command())} > {shlex.quote(os.path.relpath(self.log, ROOT))} 2>&1"


def classify(status):
    """The class of a step's exit status (`timeout` reports a child killed by signal N as 128 + N; a killed `timeout` is -N)."""
    if status == 0:
        return "ok"
    if status in (124, 137):
        return "time limit"
    if status in (134, -6):
        return "abort"
    if status in (139, -11):
        return "segmentation fault"
    return "failure"


def fault_text(log):
    with open(log, errors="replace") as f:
        text = f.read()
    return next((t for t in FAULT_TEXTS if t in text), None)


def run_chain(steps, dry_run=False):
    """Runs the steps in order and returns 0, or stops at the first one that went wrong, says which and why, and returns
    non-zero. No retry; a step after a failed one is never started."""
    if dry_run:
        print(" &&\n".join(s.shell_line() for s in steps))
        return 0
    for i, s in enumerate(steps, 1):
        os.makedirs(os.path.dirname(s.log), exist_ok=True)
        with open(s.log, "wb") as log:
            status = subprocess.run(s.command(), cwd=ROOT, env={**os.environ, **s.env}, stdin=subprocess.DEVNULL,
                                    stdout=log, stderr=subprocess.STDOUT).returncode
        found = fault_text(s.log)
        if status != 0 or found:
            what = f"fault text ({found!r}, exit status {status})" if found else f"{classify(status)} (exit status {status})"
            print(f"gpu.py: step {i} of {len(steps)} [{s.name}] ended the chain: {what}; log {os.path.relpath(s.log, ROOT)}; "
                  f"{len(steps) - i} later steps not started", file=sys.stderr, flush=True)
            return status if status > 0 else 1
        if s.then:
            s.then(s)
    return 0


# ----------------------------------------------------------------------------------------------------------- targets

BENCH_CFGS = ("c2", "c3", "c4", "c5")
SCENES = ("sand3", "sand2", "stirred", "c1", "cube64", "c4leg")       # tools/gpu_scene_prof.py


def target_command(target, bench_args, extra):
    """(argv, environment, time limit) of what `kstats` / `pmc` profile: a bench configuration, a scene of gpu_scene_prof.py
    or `native` (gpu_native_host_cost.py: one rank as its own two neighbours over RCCL). `extra` is appended to the command."""
    if target in BENCH_CFGS:
        return [PY, "bench.py", "--config", target] + bench_args + ["--no-cpu-baseline", "--no-extra", "--no-live-pmc"] + extra, {}, 300
    if target in SCENES:
        return [PY, "tools/gpu_scene_prof.py", target] + extra, {}, 300
    if target == "native":
        return [PY, "tools/gpu_native_host_cost.py"] + extra, {"HSA_ENABLE_IPC_MODE_LEGACY": "0"}, 300
    sys.exit(f"gpu.py: TARGET is one of {' '.join(BENCH_CFGS + SCENES)} native, not {target!r}")


def newest(pattern):
    files = sorted(glob.glob(pattern, recursive=True), key=os.path.getmtime)
    if not files:
        sys.exit(f"gpu.py: rocprofv3 left no {pattern}")
    return files[-1]


# ------------------------------------------------------------------------------------------------------------ kstats

def summarise_kernel_stats(out_dir):
    """rocprofv3's *_kernel_stats.csv -> out_dir/kernel_stats.csv, and one printed line per kernel."""
    src = newest(os.path.join(out_dir, "**", "*_kernel_stats.csv"))
    shutil.copyfile(src, os.path.join(out_dir, "kernel_stats.csv"))
    with open(src) as f:
        for r in csv.DictReader(f):
            print(f"{r['Name'][:100]:100s} calls {r['Calls']:>5s} avg {float(r['AverageNs'])/1e3:8.1f} min {float(r['MinNs'])/1e3:8.1f} "
                  f"max {float(r['MaxNs'])/1e3:8.1f} us  {r['Percentage']}%")


def plan_kstats(a):
    out = os.path.join(ROOT, a.out, f"kstats_{a.tag or a.target}")
    argv, env, limit = target_command(a.target, ["--steps", str(a.steps or 50), "--warmup", "10"], a.extra)

    def then(step):
        if a.target not in BENCH_CFGS:      # the scene's stats() / the substep costs the program printed last
            print(open(step.log, errors="replace").read().strip().split("\n")[-1])
        summarise_kernel_stats(out)
    return out, [Step(f"kstats {a.target}", ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"] + argv,
                      limit, os.path.join(out, "run.log"), env, then)]


# --------------------------------------------------------------------------------------------------------------- pmc

# each set is collected in a run of its own, and only --kernel-trace stands beside --pmc
COUNTER_SETS = {
    "fetch": ["FETCH_SIZE"],
    "write": ["WRITE_SIZE"],
    "sq1": ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_ANY"],
    "sq2": ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_LDS_BANK_CONFLICT", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_SALU", "SQ_WAIT_INST_LDS", "GRBM_GUI_ACTIVE", "SQ_INST_CYCLES_VMEM_RD"],
    "icache": ["SQC_ICACHE_REQ", "SQC_ICACHE_HITS", "SQC_ICACHE_MISSES", "SQC_ICACHE_MISSES_DUPLICATE", "SQC_TC_INST_REQ", "SQ_IFETCH", "SQ_WAVES", "SQ_BUSY_CYCLES"],
}


def summarise_counters(out_dir):
    """Every *_counter_collection.csv under out_dir -> out_dir/summary.json: per kernel of the library, each counter's mean
    over the second half of its launches, and what follows from them; one printed line per kernel."""
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for path in glob.glob(os.path.join(out_dir, "**", "*_counter_collection.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                acc[r["Kernel_Name"]][r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {}
    for k, cs in acc.items():
        if not k.startswith("void wgs::k_") or "k_bin" in k or "k_bodies" in k:
            continue
        e = {}
        for cn, v in cs.items():
            v = v[len(v) // 2:]
            e[cn] = sum(v) / len(v)
        if "FETCH_SIZE" in e and "WRITE_SIZE" in e:    # units of 1 KiB; FETCH_SIZE counts half on gfx950 for 16-B-per-lane streams
            e["hbm_bytes_per_launch"] = e["FETCH_SIZE"] * 2048 + e["WRITE_SIZE"] * 1024
        if "SQ_WAVE_CYCLES" in e and "SQ_WAIT_ANY" in e:
            e["wait_frac_of_wave_cycles"] = e["SQ_WAIT_ANY"] / max(e["SQ_WAVE_CYCLES"], 1)
        if "SQ_ACTIVE_INST_VALU" in e and "SQ_BUSY_CYCLES" in e:
            e["valu_active_over_busy"] = e["SQ_ACTIVE_INST_VALU"] / max(e["SQ_BUSY_CYCLES"], 1)
        out[k.split("(")[0]] = e
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, e in out.items():
        print(k[:70], {a: (round(b, 3) if b < 10 else int(b)) for a, b in e.items()})


def plan_pmc(a):
    out = os.path.join(ROOT, a.out, f"pmc_{a.tag or a.target}")
    argv, env, limit = target_command(a.target, ["--steps", str(a.steps or 12), "--warmup", "4"], a.extra)
    steps = [Step(f"pmc {a.target} {name}", ["rocprofv3", "--kernel-trace", "--pmc"] + COUNTER_SETS[name] +
                  ["--output-format", "csv", "-d", os.path.join(out, name), "--"] + argv, limit, os.path.join(out, name + ".log"), env)
             for name in a.set]
    steps[-1].then = lambda step: summarise_counters(out)
    return out, steps


# ---------------------------------------------------------------------------------------------------------------- ab

def bench_json(log):
    lines = [ln for ln in open(log, errors="replace") if ln.startswith("{")]
    if not lines:
        sys.exit(f"gpu.py: no JSON result line in {os.path.relpath(log, ROOT)}")
    return json.loads(lines[-1])


def plan_ab(a):
    """Alternating on one machine: repetition, then library, then configuration (then WGS_DEBUG bits)."""
    out = os.path.join(ROOT, a.out, a.tag or "ab")
    libs = []
    for spec in a.lib or ["tree"]:
        name, _, d = spec.partition("=")
        if not d and name != "tree":
            sys.exit(f"gpu.py: --lib {spec}: NAME=DIR, or `tree` for the in-tree libraries")
        libs.append((name, os.path.abspath(d) if d else TREE_LIBS))
    jsonl = os.path.join(out, "ab.jsonl")

    def report(rec, line):
        print(line, flush=True)
        with open(jsonl, "a") as f:
            f.write(json.dumps({**rec, "line": line}) + "\n")

    def passes_line(rec):
        def then(step):
            d = bench_json(step.log)
            rec.update(us_per_step=round(d["ms_per_step"] * 1e3, 1), passes_us={k: round(v * 1e3, 1) for k, v in d["pass_ms_per_step"].items() if v > 0.0045})
            dbg = f"dbg={rec['debug']} " if a.debug else ""
            report(rec, f"{dbg}{rec['lib']} {rec['cfg']} {rec['us_per_step']} {rec['passes_us']}")
        return then

    def legs_line(rec):
        def then(step):
            d = bench_json(step.log)
            rec.update(us_per_step=round(d["ms_per_step"] * 1e3, 1),
                       legs={k: (round(v["ms_per_step"] * 1e3, 1), round(v["roofline_g2p"]["frac"], 3)) for k, v in d["extra"].items()})
            report(rec, f"{rec['lib']} c2 {rec['us_per_step']} {rec['legs']}")
        return then

    steps = []
    for rep in range(1, (a.reps or (1 if a.legs else 2)) + 1):
        for name, d in libs:
            env = {"WGS_LIB_DIR": d}
            if a.legs:      # the default bench line with all its extra legs
                steps.append(Step(f"ab rep {rep} {name} legs", [PY, "bench.py", "--full", "--no-cpu-baseline", "--no-live-pmc"], 900,
                                  os.path.join(out, f"r{rep}_{name}_legs.log"), env, legs_line(dict(rep=rep, lib=name, cfg="c2"))))
                continue
            for cfg in a.cfg:
                for bits in ["0"] + a.debug if a.debug else [None]:
                    argv = [PY, "bench.py", "--full", "--steps", str(a.steps or 40), "--warmup", "10", "--no-cpu-baseline", "--no-extra", "--config", cfg]
                    tag = f"r{rep}_{name}_{cfg}"
                    if bits is not None:
                        argv.append("--allow-debug-switches")
                        tag += f"_dbg{bits}"
                    steps.append(Step(f"ab rep {rep} {name} {cfg}" + (f" dbg={bits}" if bits is not None else ""), argv + a.extra, 200,
                                      os.path.join(out, tag + ".log"), {**env, **({"WGS_DEBUG": bits} if bits is not None else {})},
                                      passes_line(dict(rep=rep, lib=name, cfg=cfg, debug=bits))))
    return out, steps


# ------------------------------------------------------------------------------------------------------------- tests

def plan_tests(a):
    """The -m gpu suite with the parity margins collected (tests/helpers.py report_margin; tools/summarize_margins.py)."""
    out = os.path.join(ROOT, a.out, a.tag or "tests")
    margins = os.path.join(out, "margins.jsonl")

    def then(step):
        print("".join(open(step.log, errors="replace").readlines()[-40:]), end="")
    return out, [Step("tests", [PY, "-m", "pytest", "tests", "-m", "gpu", "-q"] + a.extra, a.limit, os.path.join(out, "pytest.log"),
                      {"WGS_MARGINS_FILE": margins}, then)]


# -------------------------------------------------------------------------------------------------------------- main

def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--dry-run", action="store_true", help="print the plan as shell lines and run nothing")
    common.add_argument("--out", default="build/gpu_out", help="directory (relative to the repository) the subcommand's directory is made in")
    common.add_argument("--tag", default=None, help="name of the subcommand's directory instead of its default")
    sub = ap.add_subparsers(dest="cmd", required=True)

    p = sub.add_parser("ab", parents=[common], help="event-timed passes of bench configurations, alternating between libraries on one machine")
    p.add_argument("--lib", action="append", metavar="NAME=DIR", help="a directory with both libraries (tools/build_variant.sh); `tree` = the in-tree ones")
    p.add_argument("--cfg", nargs="+", default=["c2", "c3", "c5"], choices=BENCH_CFGS)
    p.add_argument("--reps", type=int, default=None, help="default 2 (1 with --legs)")
    p.add_argument("--steps", type=int, default=None)
    p.add_argument("--debug", nargs="+", default=[], metavar="BITS", help="each configuration with WGS_DEBUG=0 and with each of BITS")
    p.add_argument("--legs", action="store_true", help="the default bench line with its extra legs instead of --cfg")
    p.set_defaults(plan=plan_ab)

    for name, plan, text in (("kstats", plan_kstats, "rocprofv3 --kernel-trace --stats of TARGET"),
                             ("pmc", plan_pmc, "rocprofv3 counters of TARGET per kernel, one run per counter set")):
        p = sub.add_parser(name, parents=[common], help=text)
        p.add_argument("target", metavar="TARGET", help=f"{' '.join(BENCH_CFGS)} (bench.py), {' '.join(SCENES)} (gpu_scene_prof.py) or native")
        p.add_argument("--steps", type=int, default=None, help="bench steps (kstats 50, pmc 12)")
        if name == "pmc":
            p.add_argument("--set", nargs="+", default=["fetch", "write", "sq1", "sq2"], choices=tuple(COUNTER_SETS))
        p.set_defaults(plan=plan)

    p = sub.add_parser("tests", parents=[common], help="the -m gpu suite with WGS_MARGINS_FILE set")
    p.add_argument("--limit", type=int, default=2400, help="time limit of the suite in seconds")
    p.set_defaults(plan=plan_tests)

    a, extra = ap.parse_known_args(argv)        # what the subcommand does not know goes to the program it runs
    a.extra = [x for x in extra if x != "--"]
    out, steps = a.plan(a)
    if not a.dry_run:
        shutil.rmtree(out, ignore_errors=True)   # a directory per call: no summary ever mixes two runs
        os.makedirs(out)
    return run_chain(steps, a.dry_run)


if __name__ == "__main__":
    sys.exit(main())
