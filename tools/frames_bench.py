"""Cost of the coarsened flow frames (lbm_frames_begin / k_frame) against the route without them.

    python tools/frames_bench.py [--nx 4096] [--ny 1024] [--precision f64] [--arith 1] [--k 4] [--steps 2000] [--of 100]
                                 [--runs 3] [--device 0] [--once]

One JSON line from ONE context (the same binary and plan), wall times fenced by lbm_sync, each case --runs times, alternating:
  "frames":  step(--steps, --of) with frames of stride --k, then one drain_frames() of the steps / of frames;
  "plain":   the same step(--steps, --of) without frames (its force log drained outside the timing, as in the case above);
  "macros":  the route without frames: steps / of times step(--of, 0) + macros() (three full-resolution fp64 fields per picture).
The cost of a frame is (frames - plain) / (steps / of); "step_kernel_ms" is the device time of one single-iteration launch
(lbm_last_step_kernel_ms over step(64, 1) windows), the yardstick it is held against.
--once: one step(--steps, --of) + drain with frames and nothing else, for a kernel trace of the frame kernel alone.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--precision", default="f64", choices=("f64", "f32"))
    ap.add_argument("--arith", type=int, default=1)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--of", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    kw = dict(tau=0.6, inlet_velocity=100 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * args.ny))   # Re 100 on the disc, as bench.py
    nframes = args.steps // args.of
    with lbm.Context(args.nx, args.ny, device=args.device, precision=args.precision, force_log_capacity=8192, **kw) as ctx:
        ctx.set_option("arith", args.arith)
        ctx.set_option("timing", 1)
        ctx.initialise()
        ctx.step(args.of * 2, 0)
        common = {"nx": args.nx, "ny": args.ny, "precision": args.precision, "arith": "contracted" if args.arith else "strict", "k": args.k,
                  "plan": ctx.plan_options(), "kernel": ctx.kernel_name(), "build_id": lbm.build_id()}

        def with_frames():
            ctx.frames_begin(args.k, nframes + 1)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step(args.steps, args.of)
            got = ctx.drain_frames()
            dt = time.perf_counter() - t0
            ctx.frames_end()
            ctx.drain_force_log(max_rows=8192)
            assert len(got) in (nframes, nframes + 1), len(got)
            return dt

        def plain():
            ctx.sync()
            t0 = time.perf_counter()
            ctx.step(args.steps, args.of)
            ctx.sync()
            dt = time.perf_counter() - t0
            ctx.drain_force_log(max_rows=8192)
            return dt

        def by_macros():
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(nframes):
                ctx.step(args.of, 0)
                ctx.macros()
            return time.perf_counter() - t0

        if args.once:
            print(json.dumps(dict(common, case="once", seconds=round(with_frames(), 4))), flush=True)
            return
        with_frames(), plain()       # warm-up of both paths
        ctx.step(64, 1); ctx.sync(); ctx.drain_force_log(max_rows=8192)
        ctx.step(64, 1); ctx.sync(); ctx.drain_force_log(max_rows=8192)
        step_ms = ctx.last_step_kernel_ms()
        a, b, c = [], [], []
        for _ in range(args.runs):
            a.append(with_frames()); b.append(plain()); c.append(by_macros())
        ma, mb, mc = (statistics.median(v) for v in (a, b, c))
        print(json.dumps(dict(common, case="frames", steps=args.steps, output_frequency=args.of, frames_per_run=nframes,
                              seconds_frames=[round(v, 4) for v in a], seconds_plain=[round(v, 4) for v in b],
                              seconds_macros=[round(v, 4) for v in c], ms_per_frame=round((ma - mb) / nframes * 1e3, 4),
                              step_kernel_ms=round(step_ms, 4), frames_over_macros=round(ma / mc, 4),
                              first_unstable_step=ctx.first_unstable_step())), flush=True)


if __name__ == "__main__":
    main()
