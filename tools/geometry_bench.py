"""Throughput of the step kernels on user-defined geometry (lbm_set_solid_mask) against the analytic disc.

    python tools/geometry_bench.py [--nx 4096] [--ny 1024] [--steps 2000] [--warmup 1000] [--strict] [--device 0]

One JSON line per case, each on the plan the context measured for its own geometry (tune=1), fp64, contracted arithmetic unless
--strict (bench.py's setting):
    disc          the analytic disc of the cylinder_* parameters (no mask: bench.py's workload)
    disc-mask     the same disc passed as a mask (Context(solid=ctx.solid()) of an unmasked context): the mask path's own cost
    square        a square cylinder of the disc's diameter
    porous        200 random discs in a bed of 1 % random solid cells: every tile is near a solid cell (no plain-fluid path)
    porous-site   the same bed on the one-iteration site kernel (k_step_site, pinned): the floor for comparison
    disc-parabolic, disc-mask-parabolic
                  disc and disc-mask with a parabolic inlet (lbm_set_inlet_profile, parabolic_profile of the same mean velocity):
                  the per-row inlet table's cost (only the inlet column reads it)
The timed window uses bench.py's fence: warm-up, lbm_sync, then K steps that end in lbm_sync."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lbm = importlib.import_module("highperformancecomputing-latticeboltzmannmethod_amd")


def porous(nx, ny, n=200, seed=7):
    """~200 random discs (radius ny/32) in a bed of 1 % random solid cells: every 64 x 32 region holds solid cells, so no tile
    takes a plain-fluid path and every cell update looks the mask up (the mask path's worst case)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    m = (rng.random((ny, nx)) < 0.01).astype(np.uint8)
    r = max(2, ny // 32)
    for cx, cy in zip(rng.integers(nx // 16, nx - nx // 16, n), rng.integers(r + 2, ny - r - 2, n)):
        x0, x1, y0, y1 = cx - r, cx + r + 1, cy - r, cy + r + 1
        m[y0:y1, x0:x1] |= ((x[y0:y1, x0:x1] - cx) ** 2 + (y[y0:y1, x0:x1] - cy) ** 2 <= r * r)
    return m


def run(args, name, solid, kw, options=None, inlet_profile=None):
    with lbm.Context(args.nx, args.ny, device=args.device, solid=solid, options=options, inlet_profile=inlet_profile, **kw) as ctx:
        ctx.set_option("arith", 0 if args.strict else 1)
        ctx.set_option("trailing_pair", 1)
        nsolid = ctx.initialise()
        ctx.step(args.warmup, 0)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.step(args.steps, 0)
        ctx.sync()
        dt = time.perf_counter() - t0
        bad = ctx.first_unstable_step()
        line = {"case": name, "nx": args.nx, "ny": args.ny, "steps": args.steps, "warmup": args.warmup,
                "arith": "strict" if args.strict else "contracted", "glups": round(args.nx * args.ny * args.steps / dt * 1e-9, 2),
                "ms_per_step": round(dt / args.steps * 1e3, 5), "solid_cells": nsolid, "kernel": ctx.kernel_name(),
                "plan": ctx.plan_options(), "first_unstable_step": bad, "build_id": lbm.build_id()}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--strict", action="store_true", help="strict IEEE collision instead of the contracted one")
    args = ap.parse_args()
    nx, ny = args.nx, args.ny
    kw = dict(tau=0.6, inlet_velocity=100 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * ny))   # Re 100 on the disc, as bench.py
    with lbm.Context(nx, ny, device=args.device, **kw) as probe:
        disc = probe.solid()
    ys, xs = np.nonzero(disc)
    sq = np.zeros_like(disc)
    sq[ys.min():ys.max() + 1, xs.min():xs.max() + 1] = 1
    run(args, "disc", None, kw)
    run(args, "disc-mask", disc, kw)
    run(args, "square", sq, kw)
    bed = porous(nx, ny)
    run(args, "porous", bed, kw)
    # the same bed on the one-iteration site kernel (pinned plan): the floor the fused kernels must stay above
    run(args, "porous-site", bed, kw, options=dict(tune=0, layout=1, nt=1, alternate=0, fuse=1))
    prof = lbm.parabolic_profile(ny, kw["inlet_velocity"])
    run(args, "disc-parabolic", None, kw, inlet_profile=prof)
    run(args, "disc-mask-parabolic", disc, kw, inlet_profile=prof)


if __name__ == "__main__":
    main()
