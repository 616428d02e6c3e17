#!/usr/bin/env python3
"""What the wrap costs: a periodic context (lbm_set_periodic_y) against the walled one at one size, each on the plan lbm_initialise
measures for it. A periodic context is a strip with two faces: it runs the strip plans with one exchange (two device copies of its own
edge rows) per launch, where the walled context runs the whole-domain plans.

One context is alive at a time, each in a fresh child process: two contexts side by side share the process's hardware queues, and the
one created second has been seen to lose a third of its rate on plans that use two streams (profiles/ports/README.md 5b) — both the
walled context's row-range launches and the periodic context's side stream do. The children ALTERNATE (walled, periodic, walled, ...):
other people's work shares the host and the card, so a difference is read from pairs taken a moment apart; the medians over the pairs
are reported with their spread. A child times `--windows` windows of `--steps` iterations behind `--warmup` untimed ones with the host
clock around a call that ends in a device synchronise, and reports the median window. Prints one JSON line; needs a GPU (no fallback).

    python tools/periodic_bench.py --nx 4096 --ny 1024 --arith 1 --steps 20000 --pairs 3 [--out FILE]
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "highperformancecomputing-latticeboltzmannmethod_amd"
CASES = ("walled", "periodic")


def child(a):
    """One context of the case: its plan, and the rate of each window in GLUPS."""
    lbm = importlib.import_module(PKG)
    if lbm.device_count() < 1:
        sys.exit("periodic_bench: no HIP device (this measurement has no CPU fallback)")
    with lbm.Context(a.nx, a.ny, tau=0.6, inlet_velocity=0.05, precision=a.precision, options=dict(arith=a.arith),
                     periodic_y=a.case == "periodic") as c:
        c.initialise()
        c.step(a.warmup, 0)
        c.sync()
        rates = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            c.step(a.steps, 0)
            c.sync()
            rates.append(a.nx * a.ny * a.steps / (time.perf_counter() - t0) / 1e9)
        assert c.first_unstable_step() == -1
        print(json.dumps(dict(case=a.case, glups=[round(r, 2) for r in rates], glups_median=round(statistics.median(rates), 2), plan=c.plan(),
                              plan_options=c.plan_options(), kernel=c.kernel_name(), schedule=c.strip_schedule(),
                              graph_replays=c.graph_replays())))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--precision", choices=("f64", "f32"), default="f64")
    ap.add_argument("--arith", type=int, choices=(0, 1), default=1, help="0 strict, 1 contracted collision arithmetic")
    ap.add_argument("--steps", type=int, default=20000, help="iterations per timed window (about half a second at 4096x1024)")
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=5, help="timed windows per child")
    ap.add_argument("--pairs", type=int, default=3, help="alternating (walled, periodic) pairs of child processes")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--case", choices=CASES, default=None, help=argparse.SUPPRESS)      # (a child of this tool)
    a = ap.parse_args()
    if a.case:
        return child(a)
    runs = {k: [] for k in CASES}
    for pair in range(a.pairs):
        for case in CASES:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case] + [x for k in ("nx", "ny", "precision", "arith", "steps", "warmup", "windows")
                                                                               for x in ("--" + k, str(getattr(a, k)))]
            pr = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600)
            if pr.returncode != 0:
                sys.exit("periodic_bench: the %s run of pair %d ended with status %d" % (case, pair + 1, pr.returncode))
            runs[case].append(json.loads(pr.stdout.strip().splitlines()[-1]))
    out = dict(tool="periodic_bench", nx=a.nx, ny=a.ny, precision=a.precision, arith=a.arith, steps=a.steps, warmup=a.warmup,
               windows=a.windows, pairs=a.pairs)
    for case in CASES:
        med = [r["glups_median"] for r in runs[case]]
        out[case] = dict(glups_median=round(statistics.median(med), 2), glups_per_pair=med, plans=[r["plan_options"] for r in runs[case]],
                         kernel=runs[case][-1]["kernel"], plan=runs[case][-1]["plan"], schedule=runs[case][-1]["schedule"],
                         graph_replays=runs[case][-1]["graph_replays"])
    out["periodic_over_walled"] = round(statistics.median(p["glups_median"] / w["glups_median"] for p, w in zip(runs["periodic"], runs["walled"])), 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
