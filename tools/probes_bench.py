"""Cost of the point probes (lbm_probes_begin / k_probes): the time of one sample and what sampling adds to a run.

    python tools/probes_bench.py [--nx 4096] [--ny 1024] [--precision f64] [--arith 1] [--plan "layout=1 nt=1 ..."] [--n 16,4096,65536]
                                 [--frame-k 8] [--windows 7] [--samples 40] [--steps 20000] [--of 100] [--run-n 4096] [--runs 3] [--device 0]

JSON lines, all from ONE context, i.e. the same binary and plan (--plan pins it: the pairs of lbm_plan_options with tune=0):
  "sample": a window is step(S, 1) — S single-iteration launches with a force output and, with probes or frames begun, a sample each —
            timed with HIP events (option "timing"); the time per sample is the difference between the medians of --windows windows
            with and without the sample, divided by S. One line per n of --n (random points, fixed seed) and one for a frame of
            stride --frame-k, for comparison.
  "run":    step(--steps, --of) fenced by lbm_sync, --runs times without and --runs times with --run-n probes, alternating; wall time,
            GLUPS and the cost per sample (the rings are drained outside the timing).
Copied into the tree of an older commit, whose library has no probes, only the "run" line without probes is printed: the figure to hold the others against.
The flow is bench.py's (Re 100 on the disc, tau 0.6)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lbm = importlib.import_module("highperformancecomputing-latticeboltzmannmethod_amd")


def window_ms(ctx, samples):
    ctx.step(samples, 1)
    ctx.sync()
    ctx.drain_force_log(max_rows=max(4096, samples))
    return ctx.last_step_stats()[0]


def timed_run(ctx, steps, of):
    ctx.sync()
    t0 = time.perf_counter()
    ctx.step(steps, of)
    ctx.sync()
    dt = time.perf_counter() - t0
    ctx.drain_force_log(max_rows=max(4096, steps // max(of, 1) + 2))
    return dt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--precision", default="f64", choices=("f64", "f32"))
    ap.add_argument("--arith", type=int, default=1)
    ap.add_argument("--plan", default="")
    ap.add_argument("--n", default="16,4096,65536")
    ap.add_argument("--frame-k", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--of", type=int, default=100)
    ap.add_argument("--run-n", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    kw = dict(tau=0.6, inlet_velocity=100 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * args.ny))   # Re 100 on the disc, as bench.py
    cells = args.nx * args.ny
    rng = np.random.default_rng(1)
    points = lambda n: np.stack([rng.uniform(0.0, args.nx - 1.0, n), rng.uniform(0.0, args.ny - 1.0, n)], axis=1)
    with lbm.Context(args.nx, args.ny, device=args.device, precision=args.precision, force_log_capacity=8192, **kw) as ctx:
        for pair in args.plan.split():
            k, v = pair.split("=")
            ctx.set_option(k, int(v))
        if args.plan:
            ctx.set_option("tune", 0)
        ctx.set_option("arith", args.arith)
        ctx.set_option("timing", 1)
        ctx.initialise()
        ctx.step(200, 0)
        have = hasattr(ctx, "probes_begin")
        common = {"nx": args.nx, "ny": args.ny, "precision": args.precision, "arith": "contracted" if args.arith else "strict",
                  "plan": ctx.plan_options(), "kernel": ctx.kernel_name(), "build_id": lbm.build_id(), "probes_in_library": have}
        if have and args.windows > 0:
            window_ms(ctx, args.samples)                                     # warm-up of the single-iteration path
            off = [window_ms(ctx, args.samples) for _ in range(args.windows)]
            base = statistics.median(off)

            def sampled(begin, drain, end):
                begin()
                window_ms(ctx, args.samples); drain()
                on = []
                for _ in range(args.windows):
                    on.append(window_ms(ctx, args.samples)); drain()
                end()
                return on
            for n in [int(v) for v in args.n.split(",") if v]:
                xy = points(n)
                on = sampled(lambda: ctx.probes_begin(xy, args.samples), ctx.drain_probes, ctx.probes_end)
                print(json.dumps(dict(common, case="sample", what="probes", n=n, windows=args.windows, samples_per_window=args.samples,
                                      window_ms_without=[round(v, 4) for v in off], window_ms_with=[round(v, 4) for v in on],
                                      ms_per_sample=round((statistics.median(on) - base) / args.samples, 5))), flush=True)
            if args.frame_k > 0:
                on = sampled(lambda: ctx.frames_begin(args.frame_k, args.samples), ctx.drain_frames, ctx.frames_end)
                print(json.dumps(dict(common, case="sample", what="frame", k=args.frame_k, windows=args.windows, samples_per_window=args.samples,
                                      window_ms_without=[round(v, 4) for v in off], window_ms_with=[round(v, 4) for v in on],
                                      ms_per_sample=round((statistics.median(on) - base) / args.samples, 5))), flush=True)
        if args.steps > 0 and args.runs > 0:
            nsamp = args.steps // args.of + 1
            xy = points(args.run_n)
            without, with_ = [], []
            timed_run(ctx, min(args.steps, 2000), args.of)                   # warm-up of the fused path
            for _ in range(args.runs):
                without.append(timed_run(ctx, args.steps, args.of))
                if have:
                    ctx.probes_begin(xy, nsamp)
                    with_.append(timed_run(ctx, args.steps, args.of))
                    got = ctx.drain_probes()
                    assert len(got[0]) in (nsamp - 1, nsamp), len(got[0])
                    ctx.probes_end()
            glups = lambda dt: round(cells * args.steps / dt * 1e-9, 3)
            line = dict(common, case="run", steps=args.steps, output_frequency=args.of, seconds_without=[round(v, 4) for v in without],
                        glups_without=[glups(v) for v in without], first_unstable_step=ctx.first_unstable_step())
            if have:
                m0, m1 = statistics.median(without), statistics.median(with_)
                line.update(n=args.run_n, seconds_with=[round(v, 4) for v in with_], glups_with=[glups(v) for v in with_],
                            samples_per_run=args.steps // args.of, ms_per_sample_in_the_run=round((m1 - m0) / (args.steps // args.of) * 1e3, 5),
                            relative_cost=round(m1 / m0 - 1.0, 5))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
