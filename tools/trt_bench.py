"""Sustained throughput of the two-relaxation-time collision (lbm_set_trt) beside plain BGK and Smagorinsky LES, one binary.

    python tools/trt_bench.py [--nx 4096] [--ny 1024] [--steps 1000] [--warmup 1000] [--windows 5] [--magic 0.25] [--cs 0.17]

One JSON line per case: BGK, LES (constant --cs) and TRT (magic parameter --magic) in fp64 contracted, fp64 strict and fp32
(contracted) arithmetic, each on the plan its own context measured (tune=1), with the kernel that plan launches. The flow is
bench.py's (Re 100 on the disc, tau 0.6). After the warm-up, --windows timed windows of --steps steps, each fenced by lbm_sync;
the line carries every window and their median, and each TRT line the ratio of its median to the BGK median of its mode."""
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


def run(args, collision, precision, arith, kw):
    extra = dict(smagorinsky=args.cs) if collision == "les" else dict(trt_magic=args.magic) if collision == "trt" else {}
    with lbm.Context(args.nx, args.ny, device=args.device, precision=precision, **extra, **kw) as ctx:
        ctx.set_option("arith", arith)
        ctx.set_option("trailing_pair", 1)
        ctx.initialise()
        ctx.step(args.warmup, 0)
        ctx.sync()
        mlups = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            ctx.step(args.steps, 0)
            ctx.sync()
            mlups.append(args.nx * args.ny * args.steps / (time.perf_counter() - t0) * 1e-6)
        return {"case": "%s-%s-%s" % (collision, precision, "contracted" if arith else "strict"), "collision": collision,
                "precision": precision, "arith": "contracted" if arith else "strict", "nx": args.nx, "ny": args.ny,
                "steps": args.steps, "warmup": args.warmup, "mlups_windows": [round(m) for m in mlups],
                "mlups_median": round(statistics.median(mlups)), "kernel": ctx.kernel_name(), "plan": ctx.plan_options(),
                "first_unstable_step": ctx.first_unstable_step(), "build_id": lbm.build_id()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--magic", type=float, default=0.25)
    ap.add_argument("--cs", type=float, default=0.17)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    kw = dict(tau=0.6, inlet_velocity=100 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * args.ny))   # Re 100 on the disc, as bench.py
    for precision, arith in (("f64", 1), ("f64", 0), ("f32", 1)):
        bgk = None
        for collision in ("bgk", "les", "trt"):
            line = run(args, collision, precision, arith, kw)
            if collision == "bgk":
                bgk = line["mlups_median"]
            if collision == "trt":
                line["trt_over_bgk"] = round(line["mlups_median"] / bgk, 4)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
