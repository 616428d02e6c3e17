#!/usr/bin/env python3
"""bench.py — MLUPS of the D2Q9-BGK timestep (BASELINE.json metric) on N MI355X of one node.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one loop body of Solver::run (exchange + stream + BCs + stability + collision) over the whole lattice; the
library fuses up to six consecutive steps into one kernel launch (k_stepc_col: the lattice of a 64x32 region stays in
registers between them). Workload at every N: BASELINE.json configs[2], the 4096x1024 fp64 cylinder at Re=200 (tau=0.6,
u_in=0.06510417) — the grid the metric is quoted on ("4096x1024 D2Q9 at 1/2/4/8 GPUs"), so N>1 is STRONG scaling: the
rows are cut into N strips, one process per GPU, LBM_HALO_ROWS edge rows x 9 populations per face exchanged with RCCL
send/recv once per launch of six iterations (schedule measured at initialise). Populations are resident in HBM before
the timed region; nothing is copied to the host inside it and no output (forces/VTK) step falls inside it.

Runtime hygiene: liblbm_hip.so is loaded BEFORE torch (and torch only at N>1, for the gloo rendezvous of the 128-byte
ncclUniqueId and the barriers; no torch.cuda call is made), so that the process binds the ROCm RCCL/HIP the library was
built and tested against, not the copies bundled with the torch wheel; the versions actually bound are printed in the
JSON line. The timed region is bracketed by lbm_sync (both streams of the library) + a gloo barrier on both sides.

Prints ONE JSON line on rank 0 (contract in the task statement). `roofline` (dominant kernel, live HIP-event time on the
library's own stream): `achieved` / `frac` price every lattice update at SURVEY §8(d)'s 144 B (72 B fp32) exactly as the
contract defines them — above 1 for a launch that fuses d iterations, which moves ~1/d of that; `frac_hbm_measured` = the HBM
bytes the kernel really moved (committed PMC passes, profiles/traffic.json) / time / 8 TB/s; `frac_valu` = the same passes'
vector instructions against the chip's issue rate; `bound` = whichever of the two is nearer its ceiling.

A plain run does only what the headline needs: set up, warm up, time the K steps, write --dump-outputs, print the line.
Everything that takes runs of its own is behind --full: `sustained` = a second, longer window of the same context; the live
counter passes of `roofline` (without them its bytes come from profiles/traffic.json); at N=1 `cpu_baseline` (the reference
binary oracle/_ref/ref_driver if it runs on this host, else the oracle port; bounded sample), `other_arithmetic` and
`single_precision_variant` (BASELINE.json configs[4] on this GPU with its MLUPS-per-GB/s beside the fp64 figure); at N>1 the
compute-only pass of `strips` and `strips.parity`: a second short run compared bit for bit with a one-GPU run of the whole grid.

--dump-outputs DIR writes, after the timed region, what the timed calls computed: the post-collision populations of the last
timed step (a step ends on its collision; the state lbm_save_state hands a caller) at a fixed, seeded sample of lattice
sites — DIR/populations.npy [9, sites] in the run's element type and DIR/sites.npy, the sampled global site indices
y * nx + x (float64). The sample depends on the grid only, so runs of two builds, or of 1 and N GPUs, compare entry for entry.
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = "highperformancecomputing-latticeboltzmannmethod_amd"

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# vector-issue ceiling of the chip: 256 CUs x 4 SIMDs, a wave64 instruction takes 4 cycles in fp64 (16 lanes/clk/SIMD: 78.6
# TFLOP/s fp64 vector peak) and 2 in fp32 (32 lanes/clk), 2.4 GHz  ->  lane-instructions per second
VALU_LANE_RATE = {"f64": 256 * 4 * 16 * 2.4e9, "f32": 256 * 4 * 32 * 2.4e9}
BYTES_PER_LUP = {"f64": 144, "f32": 72}   # 9 loads + 9 stores per lattice update
CONFIGS = {(1024, 256, "f64", 100.0): "configs[1]", (4096, 1024, "f64", 200.0): "configs[2]", (8192, 2048, "f64", 200.0): "configs[3]",
           (16384, 4096, "f32", 200.0): "configs[4]"}


def _time_reference(ref, d, nx, ny, u_in, steps, ranks, threads, timeout=120):
    """One timed run of the unmodified reference: `ranks` MPI ranks (mpiexec) x `threads` OpenMP threads."""
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), OMP_PROC_BIND="false")
    cmd = [ref, "--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--of", "1000000", "--tau", "0.6",
           "--u", repr(u_in), "--time"]
    if ranks > 1:
        cmd = [MPIEXEC, "-n", str(ranks)] + cmd
    out = subprocess.run(cmd, cwd=d, env=env, timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    m = re.search(r"REFTIME .*ranks=(\d+) threads=(\d+) seconds=([\d.]+) mlups=([\d.]+) ok=1", out.stdout)
    if not m or int(m.group(1)) != ranks:
        raise RuntimeError((out.stderr or out.stdout)[-300:])
    return float(m.group(4))


MPIEXEC = "/opt/conda/bin/mpiexec"


def cpu_baseline(nx, ny, u_in, budget_s=12.0):
    """Reported baseline only: the reference's CPU path (MPI x OpenMP, as it ships) on this host's CPU share, bounded
    sample of the same grid. (The only place bench.py touches oracle/: the reference driver, the checker's
    thread-count helper and, as a fallback, its CPU port.)"""
    from oracle.oracle import host_cores
    cores = host_cores()
    ref = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    if os.path.exists(ref):
        try:
            import tempfile
            d = tempfile.mkdtemp(prefix="lbmref_")
            # the reference is a hybrid code; which ranks x threads split is fastest depends on the host: probe
            splits = [(1, cores)]
            if os.path.exists(MPIEXEC):
                splits += [(r, cores // r) for r in (2, 4, 8, 16, 32) if r <= cores and cores % r == 0
                           and nx % r == 0 and ny % r == 0]
            probe = {}
            for r, t in splits:
                try:
                    probe[(r, t)] = _time_reference(ref, d, nx, ny, u_in, 8, r, t, timeout=40)
                except Exception:
                    pass
            (ranks, threads) = max(probe, key=probe.get)
            # best of three runs of the chosen split (a weak baseline flatters: round 3's single 400-step run read 598 MLUPS where
            # the same split's own 8-step probe had read 732), each a third of the budget
            steps = max(5, min(200, int(budget_s / 3 * probe[(ranks, threads)] * 1e6 / (nx * ny))))
            runs = [_time_reference(ref, d, nx, ny, u_in, steps, ranks, threads) for _ in range(3)]
            return {"value": round(max(runs), 2), "unit": "MLUPS", "cores": ranks * threads, "kind": "reference",
                    "sample": f"unmodified reference (oracle/_ref/ref_driver, -O3 -ffast-math -mavx2 -mfma -fopenmp), "
                              f"{nx}x{ny} fp64, best of three runs of {steps} steps incl. its per-step stability scan "
                              f"({', '.join(f'{v:.0f}' for v in runs)} MLUPS), {ranks} MPI rank(s) x "
                              f"{threads} OpenMP threads (fastest of the probed splits: "
                              + ", ".join(f"{r}x{t}={v:.0f}" for (r, t), v in sorted(probe.items())) + " MLUPS)"}
        except Exception as e:  # the reference binary does not run on this host: time the port instead
            sys.stderr.write(f"[bench] reference binary unusable here ({e}); timing the oracle port\n")
    from oracle.oracle import Oracle, make_params
    o = Oracle(make_params(nx, ny, inlet_velocity=u_in))
    t0 = time.perf_counter(); o.run(3); dt = (time.perf_counter() - t0) / 3
    steps = max(5, min(200, int(budget_s / dt)))
    t0 = time.perf_counter(); o.run(steps); dt = time.perf_counter() - t0
    threads = o.L.lbmo_threads()
    o.close()
    return {"value": round(nx * ny * steps / dt / 1e6, 2), "unit": "MLUPS", "cores": threads, "kind": "port",
            "sample": f"oracle/lbm_oracle.c (CPU restatement, same phase structure as the reference), {nx}x{ny} fp64, "
                      f"{steps} steps, {threads} OpenMP threads"}


def _same(a, b):
    return a.replace(" ", "") == b.replace(" ", "")


def kernel_family(kernel):
    """('k_stepc_col', 'double', depth[, rows per thread, waves]) etc.: what a sibling entry may NOT differ in — only the store
    policy and the arithmetic flag may (the tall 64x48 fp32 regions <float,4,12,7,..> and the 64x32 ones <float,4,8,7,..>
    fetch 1.35 x against 1.59 x the lattice and used to count as siblings)."""
    k = kernel.replace(" ", "")
    m = re.match(r"(k_step\w*)<(\w+)", k)
    if not m:
        return (kernel, "", 0)
    shape = re.match(r"k_stepc_col<\w+,(\d+),(\d+),", k)
    return (m.group(1), m.group(2), plan_depth_of(k)) + ((int(shape.group(1)), int(shape.group(2))) if shape else ())


def measured_traffic(nx, local_ny, precision, kernel, layout="", build_id=None):
    """Fallback when the live counter passes cannot run: the committed passes of the dominant kernel on this grid
    (profiles/traffic.json; every entry carries the build id it was taken on). Exact kernel first; else the nearest sibling
    (same family, element type and depth, other store policy) flagged `approximate`. Returns (entry | None, note)."""
    tfile = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        tj = json.load(open(tfile))
    except Exception as e:
        return None, f"profiles/traffic.json unreadable ({e})"
    key = f"{nx}x{local_ny}_{precision}"
    allents = tj.get(key) or []
    ents = [dict(e) for e in allents if _same(e.get("kernel", ""), kernel)]
    approx = False
    if not ents:
        fam = kernel_family(kernel)
        arith = kernel.replace(" ", "").rstrip(">").split(",")[-1]
        sib = [dict(e) for e in allents if kernel_family(e.get("kernel", "")) == fam]
        sib.sort(key=lambda e: e.get("kernel", "").replace(" ", "").rstrip(">").split(",")[-1] != arith)   # same arithmetic first
        ents, approx = sib, True
    ents.sort(key=lambda e: e.get("layout", "") != layout)      # the pass taken in the same layout first
    if not ents:
        return None, f"no counter pass committed for {key} with {kernel} or a sibling (profiles/traffic.json)"
    e = ents[0]
    e["approximate"] = approx
    e["stale"] = bool(build_id) and e.get("build_id") != build_id
    note = e.get("source", "profiles/traffic.json") + (f" [sibling {e['kernel']}]" if approx else "")
    return e, note


PMC_GROUPS = (("FETCH_SIZE",), ("WRITE_SIZE",),
              ("SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY"))
_INIT_KERNEL = re.compile(r"k_step_site<\w+,1,")      # the collide-only launch of lbm_initialise


_LIVE_BROKEN = []      # why the live passes were given up in this run, if they were (one failure: no second attempt, no second timeout)


def live_counters(nx, ny, precision, arith, plan_options, steps, re_number=200.0, timeout=120, keep_dir=None):
    """The counter passes of THIS binary on THIS plan, taken now: tools/pmc_probe.py (same grid, plan pinned through
    lbm_plan_options, the bench's own lbm_step(steps) calls) is run as a child under `rocprofv3 --pmc`, one pass per counter
    group (FETCH_SIZE and WRITE_SIZE do not fit one pass on gfx950). Returns (entry, note) or (None, why)."""
    import glob
    import csv
    import shutil
    import tempfile
    if _LIVE_BROKEN:
        return None, "not attempted again: " + _LIVE_BROKEN[0]
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        _LIVE_BROKEN.append("rocprofv3 not found")
        return None, "rocprofv3 not found"
    probe_steps = steps if steps <= 240 else 120
    reps, warm = (6, 1) if nx * ny <= (1 << 24) else (2, 1)
    base = keep_dir or tempfile.mkdtemp(prefix="lbm_pmc_")
    tot, disp, kernels, probe = {}, {}, {}, None
    env = dict(os.environ, TMPDIR="/tmp")

    def give_up(why):      # every failure: the scratch directory goes, and no later call of this run repeats the passes
        _LIVE_BROKEN.append(why)
        if not keep_dir:
            shutil.rmtree(base, ignore_errors=True)
        return None, why
    for gi, group in enumerate(PMC_GROUPS):
        d = os.path.join(base, f"pass{gi}_{group[0].lower()}")
        cmd = [rocprof, "--pmc", *group, "-d", d, "-o", "p", "--output-format", "csv", "--", sys.executable,
               os.path.join(ROOT, "tools", "pmc_probe.py"), "--nx", str(nx), "--ny", str(ny), "--re", repr(re_number), "--precision", precision,
               "--arith", str(arith), "--plan", plan_options, "--steps", str(probe_steps), "--reps", str(reps), "--warm", str(warm)]
        try:
            out = subprocess.run(cmd, cwd="/tmp", env=env, timeout=timeout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                 start_new_session=True)
        except subprocess.TimeoutExpired:
            return give_up(f"counter pass {group[0]} timed out after {timeout} s")
        m = re.search(r'^\{"probe".*$', out.stdout, re.M)
        if out.returncode != 0 or not m:
            return give_up(f"counter pass {group[0]} failed (rc {out.returncode}): {(out.stderr or out.stdout)[-200:]}")
        probe = json.loads(m.group(0))
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            return give_up(f"counter pass {group[0]} wrote no counter_collection.csv")
        for f in files:
            with open(f, newline="") as fh:
                for r in csv.DictReader(fh):
                    k = re.sub(r"\(.*$", "", re.sub(r"^void ", "", r["Kernel_Name"])).replace("lbmk::", "").replace(" ", "")
                    if not k.startswith("k_step") or _INIT_KERNEL.match(k):
                        continue
                    c = r["Counter_Name"]
                    tot[c] = tot.get(c, 0.0) + float(r["Counter_Value"])
                    disp[c] = disp.get(c, 0) + 1
                    kernels.setdefault(c, {}).setdefault(k, 0)
                    kernels[c][k] += 1
    if not keep_dir:
        shutil.rmtree(base, ignore_errors=True)
    if "FETCH_SIZE" not in tot or "WRITE_SIZE" not in tot or not probe:
        return give_up("counter passes returned no FETCH_SIZE / WRITE_SIZE rows for the step kernels")
    launches = probe["launches"]
    if disp["FETCH_SIZE"] != launches or disp["WRITE_SIZE"] != launches:
        return give_up(f"dispatch count mismatch: probe issued {launches} step launches, passes saw {disp['FETCH_SIZE']} / {disp['WRITE_SIZE']}")
    fetch = tot["FETCH_SIZE"] * 1024 * 2 / launches      # KiB -> B; x2: gfx950 tallies the 128-B requests of a coalesced read stream at 64 B
    write = tot["WRITE_SIZE"] * 1024 / launches
    e = {"kernel": probe["kernel"], "hbm_bytes_per_launch": int(fetch + write), "fetch_bytes_corrected": int(fetch), "write_bytes": int(write),
         "launches_sampled": launches, "iterations_per_launch": probe["iterations"] / launches, "build_id": probe["build_id"],
         "kernels_sampled": kernels["FETCH_SIZE"], "stale": False, "approximate": False, "probe_steps_per_call": probe_steps,
         "method": "live: tools/pmc_probe.py (plan pinned by lbm_plan_options) as a child under rocprofv3 --pmc, one pass per counter group; "
                   "KiB -> B; FETCH_SIZE x2 (gfx950 correction, MI355X_MICROARCH.md HBM section)"}
    for c, name in (("SQ_INSTS_VALU", "valu_insts_per_launch"), ("SQ_INSTS_LDS", "lds_insts_per_launch"), ("SQ_ACTIVE_INST_VALU", "active_inst_valu"),
                    ("SQ_BUSY_CYCLES", "busy_cycles"), ("SQ_WAVE_CYCLES", "wave_cycles"), ("SQ_WAIT_ANY", "wait_any")):
        if c in tot:
            e[name] = tot[c] / launches
    return e, "live counter passes of this binary and plan (rocprofv3 --pmc around tools/pmc_probe.py, taken after the timed region)"


def plan_depth_of(kernel):
    m = re.match(r"k_step(\d)_tile|k_stepd_tile<\w+,\d+,\d+,(\d)|k_stepc_col<\w+,\d+,\d+,(\d)", kernel)
    return int(next(g for g in m.groups() if g)) if m else 1


def roofline_of(lbm, ctx, nx, local_ny, precision, kernel_ms, launches, iterations, steps, arith=1, live=True, re_number=200.0):
    """The `roofline` object for the dominant kernel of a timed call (see the module docstring)."""
    bpl = BYTES_PER_LUP[precision]
    ipl = iterations / max(launches, 1)
    launch_bytes = int(nx * local_ny * bpl * ipl)          # 144 B (72 B) x the lattice updates of one launch
    kernel = ctx.kernel_name()
    build_id = lbm.build_id()
    ent = None
    tnote = "live counter passes not requested"
    if live:
        ent, tnote = live_counters(nx, local_ny, precision, arith, " ".join(f"{k}={v}" for k, v in ctx.plan_options().items()), steps, re_number)
    if ent is None:
        live_note = tnote
        ent, tnote = measured_traffic(nx, local_ny, precision, kernel, ctx.plan().split("/")[0], build_id)
        tnote += f" (live passes: {live_note})"
    secs = kernel_ms * 1e-3
    achieved = launch_bytes / secs / 1e9 if secs > 0 else 0.0
    r = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None, "kernel": kernel, "kernel_ms": round(kernel_ms, 5),
         "algorithmic_bytes_per_launch": launch_bytes, "iterations_per_launch": round(ipl, 4),
         "frac_144B": round(achieved / HBM_PEAK_GBS, 4), "frac_hbm_measured": None, "frac_valu": None,
         "frac_hbm_fused_minimum": round((launch_bytes / ipl) / secs / 1e9 / HBM_PEAK_GBS, 4) if secs > 0 else None,
         "traffic_source": tnote}
    if ent:
        # bytes per launch as the passes counted them, at the launch depth(s) they were taken at: a fused launch moves about one
        # read and one write of the lattice whatever its depth, so nothing is rescaled by depth; the live passes
        # replay the timed call's own launch mix
        traffic = int(ent["hbm_bytes_per_launch"])
        ipl_t = float(ent.get("iterations_per_launch") or ipl)
        gbs = traffic / secs / 1e9
        r.update(traffic=traffic, traffic_iterations_per_launch=round(ipl_t, 4), hbm_gbs_measured=round(gbs, 1),
                 frac_hbm_measured=round(gbs / HBM_PEAK_GBS, 4),
                 hbm_bytes_per_update=round(traffic / (nx * local_ny * ipl_t), 2),
                 mlups_per_gbs=round(1000.0 / (traffic / (nx * local_ny * ipl_t)), 2),
                 traffic_build_id=ent.get("build_id"), stale=bool(ent.get("stale")), approximate=bool(ent.get("approximate")),
                 fetch_bytes_corrected=ent.get("fetch_bytes_corrected"), write_bytes=ent.get("write_bytes"))
        if ent.get("valu_insts_per_launch"):
            lane = ent["valu_insts_per_launch"] * 64.0 / (nx * local_ny * ipl_t)      # lane-instructions per lattice update
            ceil = VALU_LANE_RATE[precision] / lane / 1e6                              # MLUPS if vector issue were the only limit
            r.update(valu_lane_instr_per_update=round(lane, 1), valu_ceiling_mlups=round(ceil, 0),
                     frac_valu=round(nx * local_ny * ipl / secs / 1e6 / ceil, 4),
                     lds_insts_per_update=round(ent.get("lds_insts_per_launch", 0) * 64.0 / (nx * local_ny * ipl_t), 2))
        if r["frac_valu"] and r["frac_valu"] > r["frac_hbm_measured"]:
            r["bound"] = "valu"      # (the contract's vocabulary has no word for it: vector issue, no MFMA on this path)
    r["note"] = ("achieved/frac = frac_144B: SURVEY 8(d)'s algorithmic bytes (144 B fp64 / 72 B fp32 per lattice update) x the updates of "
                 "one launch / the kernel's live launch time / 8 TB/s — ABOVE 1 because a launch fuses iterations_per_launch "
                 "iterations in registers and so moves ~1/d of the unfused bytes; it is the figure to hold against an unfused "
                 "kernel's roofline (north_star's 70 % = 0.70). frac_hbm_measured = bytes the kernel really moved (PMC FETCH_SIZE x2 + "
                 "WRITE_SIZE, separate passes taken by this run on this binary and plan: traffic_source) / time / 8 TB/s (the streaming ceiling "
                 "measured on this part is 6.0-6.3 TB/s = 0.75-0.79); frac_valu = vector lane-instructions per update from the SQ pass against "
                 "1024 SIMDs x 16 (fp64) or 32 (fp32) lanes/clk x 2.4 GHz (the chip holds ~1.9 GHz under this load: profiles/r04); "
                 "bound = the larger of the two; frac_hbm_fused_minimum = one read + one write of the lattice per launch, the least any "
                 "d-iteration launch can move")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--nx", type=int, default=4096)
    ap.add_argument("--ny", type=int, default=1024)
    ap.add_argument("--re", type=float, default=200.0)
    ap.add_argument("--precision", choices=["f64", "f32"], default="f64")
    ap.add_argument("--arith", choices=["contracted", "strict"], default="contracted",
                    help="collision arithmetic: contracted = FMA + one reciprocal (what the reference's -ffast-math -mfma build "
                         "permits; rho/u within 1e-10 of the reference, tests), strict = IEEE op by op (bit-identical to the CPU oracle)")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong",
                    help="strong: the named grid cut into N strips (BASELINE metric); weak: ny rows PER GPU")
    ap.add_argument("--set", action="append", default=[], help="library option key=value (lbm_set_option), e.g. deep=7")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-arith", action="store_true", help="skip the run in the other arithmetic mode (profiler passes)")
    ap.add_argument("--no-sustained", action="store_true", help="skip the second, longer window (profiler passes)")
    ap.add_argument("--no-f32-variant", action="store_true", help="skip the single-precision variant (BASELINE.json configs[4]) beside the headline")
    ap.add_argument("--no-live-pmc", action="store_true", help="do not take the counter passes (rocprofv3 child runs after the timed region): "
                                                               "roofline.traffic then comes from profiles/traffic.json")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what takes runs of its own: the sustained window, the live counter passes, the other "
                         "arithmetic, the fp32 variant and the CPU baseline (N=1), the compute-only pass and the strip parity (N>1); "
                         "the --no-* options above switch parts of it off")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's populations (a fixed, seeded sample of sites) as DIR/*.npy")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one process per GPU)")
        args.gpus = world

    # the HIP library first: it brings in /opt/rocm's RCCL and HIP runtime before anything else can
    lbm = importlib.import_module(PKG)
    lbm.lib()
    if lbm.device_count() < 1:
        sys.exit("no HIP device: the HIP path has no CPU fallback")
    versions = lbm.runtime_versions()
    dist = torch = None
    if world > 1:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(minutes=10))
    ndev = lbm.device_count()
    device = local_rank % ndev          # (a launcher may expose one device per rank)
    exit_code = 0

    nx = args.nx
    ny_total = args.ny * (world if args.scaling == "weak" else 1)
    if ny_total % world:
        sys.exit(f"ny={ny_total} not divisible by {world} strips")
    local_ny = ny_total // world
    # keep tau = 0.6 (nu = 1/30) and set u_in so that params.reynolds() == Re
    u_in = args.re * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * ny_total)

    ctx = lbm.Context(nx, ny_total, tau=0.6, inlet_velocity=u_in, y_start=rank * local_ny, local_ny=local_ny,
                      precision=args.precision, device=device)
    ctx.set_option("arith", 1 if args.arith == "contracted" else 0)
    ctx.set_option("trailing_pair", 1)      # the bench reads no snapshot: a call may end on a fused launch
    for kv in args.set:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    if world > 1:
        ident = [ctx.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(ident, src=0)
        ctx.comm_init(rank, world, ident[0])
    ctx.initialise()
    ctx.set_option("timing", 1)

    def fence():
        # Device side: lbm_sync drains both streams of the library — every kernel and every exchange of this process lives
        # on them. (torch.cuda.synchronize() is not an option here: with the ROCm runtime of the library resident, the torch
        # wheel's own HIP initialisation finds no device — torch is used for the gloo rendezvous and barriers only.)
        ctx.sync()
        if world > 1:
            dist.barrier()

    ctx.step(args.warmup, 0)
    fence()
    t0 = time.perf_counter()
    ctx.step(args.steps, 0)
    t_issue = time.perf_counter() - t0      # what the host needed to ISSUE the window (launches, events, exchanges): the floor of a host-bound strip
    fence()
    dt = time.perf_counter() - t0
    ms_total, launches, iterations = ctx.last_step_stats()
    kernel_ms = ms_total / max(launches, 1)            # mean duration of one launch of the dominant kernel
    if args.dump_outputs:      # (before anything below advances or re-initialises the context)
        dump_outputs(ctx, args.dump_outputs, nx, ny_total, rank * local_ny, local_ny, args.precision, dist, rank, world)
    # `sustained`: a second, longer window of the same context (the driver's K may be as short as 20 steps = 4 launches,
    # which a boosting clock flatters by ~5 %): at least 3000 steps / 80 ms
    sus_steps = max(3000, args.steps) if world == 1 else max(1200, args.steps)
    dt_sus = None
    if args.full and not args.no_sustained:
        t1 = time.perf_counter()
        ctx.step(sus_steps, 0)
        fence()
        dt_sus = time.perf_counter() - t1
    compute_only_ms = None
    if world > 1:
        tt = torch.tensor([dt, kernel_ms, dt_sus or 0.0, t_issue], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt, kernel_ms, dt_sus, t_issue = float(tt[0]), float(tt[1]), (float(tt[2]) if dt_sus else None), float(tt[3])
    graph_replays = ctx.graph_replays()
    bad = ctx.first_unstable_step()
    if bad != -1:
        sys.exit(f"simulation unstable at timestep {bad}: result invalid")
    # what ran in the timed region (the parity pass below initialises the context again)
    kernel, plan_used, schedule_used = ctx.kernel_name(), ctx.plan(), ctx.strip_schedule()
    plan_pairs = " ".join(f"{k}={v}" for k, v in ctx.plan_options().items())      # `--set tune=0 --set <pair> ...` reproduces the plan in another run
    arith_id = 1 if args.arith == "contracted" else 0
    roof = roofline_of(lbm, ctx, nx, local_ny, args.precision, kernel_ms, launches, iterations, args.steps, arith_id,
                       live=(world == 1 and args.full and not args.no_live_pmc), re_number=args.re) if rank == 0 else None
    parity = None
    if world > 1 and args.full:
        # what the halo traffic costs: the same launches with the exchange skipped (diagnostic pass, results discarded)
        n = max(60, min(args.steps, 600))
        ctx.set_option("skip_exchange", 1)
        ctx.step(30, 0)
        fence()
        t1 = time.perf_counter()
        ctx.step(n, 0)
        fence()
        tt = torch.tensor([(time.perf_counter() - t1) / n * 1e3], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        compute_only_ms = float(tt[0])
        ctx.set_option("skip_exchange", 0)
        parity = strip_parity(lbm, ctx, dist, rank, world, nx, ny_total, local_ny, u_in, args, device)

    other = None
    spv = None
    if world == 1 and args.full and not args.no_other_arith:
        # the same workload in the OTHER arithmetic mode, same harness, reported beside the headline (not part of `value`)
        oa = "strict" if args.arith == "contracted" else "contracted"
        with lbm.Context(nx, ny_total, tau=0.6, inlet_velocity=u_in, precision=args.precision, device=device,
                         options=dict(arith=1 if oa == "contracted" else 0, trailing_pair=1)) as c2:
            c2.initialise()
            c2.step(args.warmup, 0)
            c2.sync()
            t1 = time.perf_counter()
            c2.step(sus_steps, 0)
            c2.sync()
            dt2 = time.perf_counter() - t1
            ub = c2.first_unstable_step()
            if ub != -1:
                sys.exit(f"the {oa} run went unstable at timestep {ub}: result invalid")
            other = {"arithmetic": oa, "value": round(nx * ny_total * sus_steps / dt2 / 1e6, 1), "unit": "MLUPS", "steps": sus_steps,
                     "kernel": c2.kernel_name(), "plan": c2.plan(), "unstable": ub}
    if world == 1 and args.full and not args.no_f32_variant and (nx, ny_total, args.precision) == (4096, 1024, "f64"):
        spv = single_precision_variant(lbm, device, args)

    if rank == 0:
        cells = nx * ny_total
        mlups = cells * args.steps / dt / 1e6
        hr = lbm.Context.HALO_ROWS
        cfg_name = CONFIGS.get((nx, ny_total, args.precision, float(args.re)))
        line = {
            "metric": f"MLUPS ({'fp64' if args.precision == 'f64' else 'fp32'})", "value": round(mlups, 1), "unit": "MLUPS", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 5), "higher_is_better": True,
            "scaling": args.scaling, "vs_baseline": None,
            "dtype": args.precision, "data": "synthetic",
            "config": {"workload": f"D2Q9-BGK cylinder Re={args.re:g}, {nx}x{ny_total} {args.precision}, tau=0.6, u_in={u_in:.8f}"
                                   + (f" (BASELINE.json {cfg_name})" if cfg_name else " (not a BASELINE.json config)"),
                       "nx": nx, "ny": ny_total, "rows_per_gpu": local_ny, "decomposition": f"{world} row strip(s)",
                       "arithmetic": ("FMA-contracted collision, one reciprocal (as the reference's -ffast-math -mfma build permits; rho/u within "
                                      "1e-10 of the reference)" if args.arith == "contracted" else
                                      "strict IEEE, operation by operation (populations bit-identical to the CPU oracle)"),
                       "halo": "none" if world == 1 else f"RCCL send/recv of {hr} edge rows x 9 populations per face (one contiguous message "
                                                          f"of {hr * 9} sub-rows); schedule: {schedule_used}",
                       "kernel": kernel, "plan": plan_used, "plan_options": plan_pairs, "build_id": lbm.build_id(),
                       "runtime": {"rccl": versions["rccl"], "hip_runtime": versions["hip_runtime"], "hip_driver": versions["hip_driver"],
                                   "torch_loaded": torch is not None}},
            "roofline": roof,
        }
        if dt_sus:
            line["sustained"] = {"value": round(cells * sus_steps / dt_sus / 1e6, 1), "unit": "MLUPS", "steps": sus_steps,
                                 "ms_per_step": round(dt_sus / sus_steps * 1e3, 5),
                                 "note": "a second, longer window of the same context, same fences; `value` above is the contract's K-step window. "
                                         "Why a short window reads lower (profiles/r04/README.md, kernel trace of the driver's call): K = 20 is three "
                                         "launches, 6+7+7 — the seven-iteration launches a remainder needs run 3-4 % slower per iteration than the plan's "
                                         "six, the first launch after the fence another ~4 % (idle chip), and ~20 us of fence-to-first-kernel and "
                                         "completion-to-host latency fall inside a 0.54 ms window; there is no gap between the kernels"}
        if world > 1:
            graph_opt = next((int(kv.split("=")[1]) for kv in args.set if kv.startswith("graph=")), 1)
            line["strips"] = {"nranks": world, "schedule": schedule_used,
                              # slowest rank: host time to issue one iteration's share of launches / events / exchanges in the timed window
                              "host_issue_us_per_iteration": round(t_issue / args.steps * 1e6, 3),
                              "gpu_us_per_iteration": round(dt / args.steps * 1e6, 3),
                              # hipGraph replay of the launch groups: between real peers only on request (--set graph=2; never run
                              # between two GPUs so far: DESIGN §5 says what to expect with and without it)
                              "graph": ("replayed" if graph_replays > 0 else ("off (multi-rank default; --set graph=2 asks for it)" if graph_opt < 2 else
                                        "refused: launch groups issued call by call")),
                              "graph_replays_rank0": graph_replays,
                              # (from the library's own description of the measured schedule: six rows per launch or twelve per two)
                              "halo_bytes_per_face_and_exchange": (lambda m: int(m.group(1)) if m else None)(re.search(r"(\d+) B per face and exchange", schedule_used))}
            if compute_only_ms is not None:
                line["strips"].update(ms_per_step_compute_only=round(compute_only_ms, 5),
                                      ms_per_step_exchange_exposed=round(dt / args.steps * 1e3 - compute_only_ms, 5))
            line["strips"].update(parity or {"parity": "not checked (--full compares the strips with a one-GPU run)"})
            verdict = str(line["strips"]["parity"])
            if verdict.startswith("MISMATCH"):
                line["value_unverified"] = line["value"]
                line["value"] = None            # as for an unstable run: a wrong halo exchange has no throughput
            elif verdict != "bit-equal":
                line["parity_unverified"] = True
        if other is not None:
            line["other_arithmetic"] = other
        if spv is not None:
            if roof.get("mlups_per_gbs"):
                spv["mlups_per_gbs_fp64_headline"] = roof["mlups_per_gbs"]
            line["single_precision_variant"] = spv
        if world == 1 and args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(nx, ny_total, u_in)
        print(json.dumps(line), flush=True)
        if world > 1:
            verdict = str((parity or {}).get("parity", ""))
            if verdict.startswith("MISMATCH"):
                sys.stderr.write(f"[bench] strips do not reproduce the one-GPU run ({verdict}): the line above is INVALID\n")
                exit_code = 3
    ctx.close()
    if world > 1:
        code = torch.tensor([exit_code], dtype=torch.int32)
        dist.all_reduce(code, op=dist.ReduceOp.MAX)          # every rank leaves with rank 0's verdict
        exit_code = int(code[0])
        dist.barrier()
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


def single_precision_variant(lbm, device, args):
    """north_star / BASELINE.json configs[4]: the fp32 variant (16384x4096, Re=200) on this one GPU (2 x 2.4 GB), with its
    MLUPS per GB/s of HBM traffic to hold beside the fp64 figure (the 8-GPU strip run of that grid is the driver's)."""
    nx, ny = 16384, 4096
    u_in = 200.0 * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * ny)
    steps = 600
    try:
        with lbm.Context(nx, ny, tau=0.6, inlet_velocity=u_in, precision="f32", device=device,
                         options=dict(arith=1 if args.arith == "contracted" else 0, trailing_pair=1)) as c:
            c.initialise()
            c.set_option("timing", 1)
            c.step(60, 0)
            c.sync()
            t1 = time.perf_counter()
            c.step(steps, 0)
            c.sync()
            dt = time.perf_counter() - t1
            if c.first_unstable_step() != -1:
                return {"error": "unstable"}
            ms_total, launches, iterations = c.last_step_stats()
            roof = roofline_of(lbm, c, nx, ny, "f32", ms_total / max(launches, 1), launches, iterations, steps, 1 if args.arith == "contracted" else 0,
                               live=not args.no_live_pmc)
            out = {"workload": f"D2Q9-BGK cylinder Re=200, {nx}x{ny} f32 (BASELINE.json configs[4]) on ONE GPU", "value": round(nx * ny * steps / dt / 1e6, 1),
                   "unit": "MLUPS", "steps": steps, "kernel": c.kernel_name(), "plan": c.plan()}
            for k in ("frac_144B", "frac_hbm_measured", "frac_valu", "hbm_gbs_measured", "hbm_bytes_per_update", "mlups_per_gbs", "bound", "traffic",
                      "traffic_source", "traffic_build_id", "stale", "approximate", "kernel_ms", "iterations_per_launch"):
                out[k] = roof.get(k)
            return out
    except Exception as e:      # (a GPU that cannot hold 2 x 2.4 GB beside the headline context: report, do not fail the bench)
        return {"error": str(e)[:200]}


DUMP_SITES = 1 << 19          # sampled sites of --dump-outputs: 9 x 2^19 fp64 populations = 38 MB (+ 4 MB of indices), under 64 MB
DUMP_SEED = 20261016


def dump_sites(nx, ny):
    """The sorted global site indices (y * nx + x) --dump-outputs samples: every site of a small grid, else DUMP_SITES drawn
    without replacement by a generator of fixed seed — a function of the grid alone."""
    import numpy as np
    n = nx * ny
    if n <= DUMP_SITES:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=DUMP_SITES, replace=False))


def dump_outputs(ctx, out_dir, nx, ny_total, y_start, local_ny, precision, dist, rank, world):
    """--dump-outputs: the post-collision populations of the last timed step at the sampled sites, read through
    lbm_save_state (the one accessor that needs no extra step after a call that ended on a fused launch; layout: a header,
    then [9][local_ny][nx] in the element type). Each rank reads its own rows; rank 0 writes the strips' samples in row order."""
    import numpy as np
    sites = dump_sites(nx, ny_total)
    mine = sites[(sites >= y_start * nx) & (sites < (y_start + local_ny) * nx)]
    os.makedirs(out_dir, exist_ok=True)
    ckpt = os.path.join(out_dir, f".state_rank{rank}.ckpt")
    try:
        ctx.save_state(ckpt)
        dtype = np.float64 if precision == "f64" else np.float32
        body = 9 * local_ny * nx * np.dtype(dtype).itemsize
        f = np.memmap(ckpt, dtype=dtype, mode="r", offset=os.path.getsize(ckpt) - body, shape=(9, local_ny * nx))
        vals = np.array(f[:, mine - y_start * nx])
        del f
    finally:
        if os.path.exists(ckpt):
            os.remove(ckpt)
    if world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, vals)
        vals = np.concatenate(parts, axis=1)      # rank r holds rows [r * local_ny, (r + 1) * local_ny): row order
    if rank == 0:
        assert vals.shape == (9, sites.size), (vals.shape, sites.size)
        np.save(os.path.join(out_dir, "populations.npy"), vals)
        np.save(os.path.join(out_dir, "sites.npy"), sites.astype(np.float64))


def row_checksums(populations):
    """Exact per-row checksum of a [rows, nx+2, 9] float64 array: the sum of the bit patterns modulo 2**64."""
    import numpy as np
    a = np.ascontiguousarray(populations, dtype=np.float64)
    return a.view(np.uint64).reshape(a.shape[0], -1).sum(axis=1, dtype=np.uint64)


def compare_row_checksums(gathered, whole_sums):
    """'bit-equal', or where the strips' rows first differ from the whole-grid run. gathered: one dict per rank with `rank`,
    `y_start`, `rows` and `sums` (the strip's per-row checksums)."""
    import numpy as np
    for g in sorted(gathered, key=lambda g: g["rank"]):
        got = np.array(g["sums"], dtype=np.uint64)
        ref = np.asarray(whole_sums, dtype=np.uint64)[g["y_start"]:g["y_start"] + g["rows"]]
        if got.shape != ref.shape:
            return f"MISMATCH: rank {g['rank']} reports {got.shape[0]} rows, the whole grid has {ref.shape[0]} there"
        diff = np.nonzero(got != ref)[0]
        if diff.size:
            return f"MISMATCH: rank {g['rank']} first differs at global row {g['y_start'] + int(diff[0])} ({diff.size} of {g['rows']} rows)"
    return "bit-equal"


def strip_parity(lbm, ctx, dist, rank, world, nx, ny_total, local_ny, u_in, args, device):
    """Outside the timed region: a SECOND short run from iteration 0 on the strips (same communicator, same measured plan and
    schedule: lbm_initialise again), whose post-collision populations are compared row by row, bit for bit, with a one-GPU
    run of the whole grid made by rank 0 on its own device — strips must reproduce the one-rank result exactly, in either
    arithmetic mode (tests/), so the first N>1 line proves exchange_rccl's nranks>1 branch (csrc/lbm_hip.hip; replaces the
    reference's Grid::exchange_ghost_cells, LBMGrid.h:249-283) by itself."""
    import numpy as np
    # long enough that a graph-replaying schedule (option graph=2: four launch groups per replay, captured after a first eager
    # stretch) is compared too: 2 x 4 groups x 6 iterations + 4 x 6 + 1, rounded up; odd, so the call ends on a single iteration
    its = 97
    try:      # (whatever goes wrong on a rank, it still takes part in the gather below: nobody is left waiting)
        ctx.set_option("trailing_pair", 0)      # the call ends on a single iteration: f_next can be read back
        ctx.initialise()                         # collective (the strip schedule is re-measured): every rank is here
        ctx.step(its, 0)
        ctx.sync()
        sums = row_checksums(ctx.populations("f_next")[1:-1])    # (local_ny, nx+2, 9): the strip's own rows, ghost columns included
        info = dict(rank=rank, y_start=rank * local_ny, rows=local_ny, plan=ctx.plan(), schedule=ctx.strip_schedule(),
                    kernel=ctx.kernel_name(), unstable=ctx.first_unstable_step(), sums=sums.tolist())
    except Exception as e:
        info = dict(rank=rank, y_start=rank * local_ny, rows=local_ny, plan="", schedule="", kernel="", unstable=None, sums=None,
                    error=f"{type(e).__name__}: {e}"[:300])
    gathered = [None] * world
    dist.all_gather_object(gathered, info)
    if rank != 0:
        return {}
    errors = [f"rank {g['rank']}: {g['error']}" for g in gathered if g.get("error")]
    wplan = ""
    if errors:
        verdict = "unavailable (" + "; ".join(errors) + ")"
    else:
        try:
            with lbm.Context(nx, ny_total, tau=0.6, inlet_velocity=u_in, precision=args.precision, device=device,
                             options=dict(arith=1 if args.arith == "contracted" else 0)) as whole:
                whole.initialise()
                whole.step(its, 0)
                wsums = row_checksums(whole.populations("f_next")[1:-1])
                wplan = whole.plan()
            verdict = compare_row_checksums(gathered, wsums)
        except Exception as e:
            verdict = f"unavailable (whole-grid run on rank 0: {type(e).__name__}: {e})"[:400]
    return {"parity": verdict,
            "parity_basis": f"{its} iterations from initialise on the {world} strips vs one whole-grid context on rank 0's GPU ({wplan}); "
                            f"per-row checksums of the f_next bit patterns, gathered over gloo",
            "per_rank": [dict(rank=g["rank"], rows=g["rows"], plan=g["plan"], schedule=g["schedule"], kernel=g["kernel"],
                              unstable=g["unstable"]) for g in sorted(gathered, key=lambda g: g["rank"])]}


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException as e:   # one failing rank must not leave the others waiting at a barrier
        import traceback
        traceback.print_exc()
        sys.stderr.write(f"[bench] rank {os.environ.get('RANK', '0')} failed: {e}\n")
        sys.stderr.flush()
        os._exit(1)
