"""Cost of the time-averaged statistics (lbm_stats_begin / k_stats): the time of one sample and what sampling adds to a run.

    python tools/stats_bench.py [--nx 4096] [--ny 1024] [--precision f64] [--arith 1] [--windows 7] [--samples 40]
                                [--steps 20000] [--of 100] [--runs 3] [--device 0]

Two JSON lines, both from ONE context, i.e. the same binary and plan:
  "sample": a window is step(S, 1) — S single-iteration launches with a force output and, with statistics begun, a sample each —
            timed with HIP events (option "timing"); the time per sample is the difference between the medians of --windows windows
            with and without statistics, divided by S. Reported with the bytes a sample moves (9 sizeof(T) + 96 per cell) as TB/s.
  "run":    step(--steps, --of) fenced by lbm_sync, --runs times without and --runs times with statistics, alternating; wall time,
            GLUPS and the relative cost of sampling every --of steps.
The flow is bench.py's (Re 100 on the disc, tau 0.6)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--of", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    kw = dict(tau=0.6, inlet_velocity=100 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * args.ny))   # Re 100 on the disc, as bench.py
    esize = 8 if args.precision == "f64" else 4
    cells = args.nx * args.ny
    sample_bytes = cells * (9 * esize + 96)
    with lbm.Context(args.nx, args.ny, device=args.device, precision=args.precision, force_log_capacity=8192, **kw) as ctx:
        ctx.set_option("arith", args.arith)
        ctx.set_option("timing", 1)
        ctx.initialise()
        ctx.step(200, 0)
        common = {"nx": args.nx, "ny": args.ny, "precision": args.precision, "arith": "contracted" if args.arith else "strict",
                  "plan": ctx.plan_options(), "kernel": ctx.kernel_name(), "build_id": lbm.build_id()}
        ctx.stats_end()
        window_ms(ctx, args.samples)                                     # warm-up of the single-iteration path
        off = [window_ms(ctx, args.samples) for _ in range(args.windows)]
        ctx.stats_begin(0)
        window_ms(ctx, args.samples)
        on = [window_ms(ctx, args.samples) for _ in range(args.windows)]
        per = (statistics.median(on) - statistics.median(off)) / args.samples
        print(json.dumps(dict(common, case="sample", windows=args.windows, samples_per_window=args.samples,
                              window_ms_without=[round(v, 4) for v in off], window_ms_with=[round(v, 4) for v in on],
                              ms_per_sample=round(per, 5), bytes_per_sample=sample_bytes,
                              tb_per_s=round(sample_bytes / (per * 1e-3) * 1e-12, 3) if per > 0 else None)), flush=True)
        if args.steps > 0 and args.runs > 0:
            without, with_ = [], []
            timed_run(ctx, min(args.steps, 2000), args.of)                   # warm-up of the fused path
            for _ in range(args.runs):
                ctx.stats_end()
                without.append(timed_run(ctx, args.steps, args.of))
                ctx.stats_begin(0)
                with_.append(timed_run(ctx, args.steps, args.of))
            glups = lambda dt: round(cells * args.steps / dt * 1e-9, 2)
            m0, m1 = statistics.median(without), statistics.median(with_)
            print(json.dumps(dict(common, case="run", steps=args.steps, output_frequency=args.of,
                                  seconds_without=[round(v, 4) for v in without], seconds_with=[round(v, 4) for v in with_],
                                  glups_without=[glups(v) for v in without], glups_with=[glups(v) for v in with_],
                                  samples_per_run=args.steps // args.of,
                                  relative_cost=round(m1 / m0 - 1.0, 5), first_unstable_step=ctx.first_unstable_step())), flush=True)


if __name__ == "__main__":
    main()
