"""Time-dependent inlet schedules (lbm_set_inlet_schedule, Context/Group(inlet_schedule=...), lbm_solver --inlet-ramp / --inlet-pulse /
--inlet-schedule) on the GPU.

The Zou-He inlet of iteration t imposes u[y] * s(t), one IEEE multiplication in the element type; every fused level of a launch takes
the factor of its own iteration, and so does a launch replayed from a graph. The reference is oracle_run(schedule=...) of
tests/reference.py (the stepwise oracle, whose boundary step takes the scaled inlet): strict fp64 plans must match it bit for bit."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PLANS, TALL_F32, assert_group_is_whole, assert_matches_reference, assert_same_results,  # noqa: F401
                           host_staged_two_strips, lbm_gpu, masks, read_csv_rows, read_params, read_velocity_field, record, run_ctx, run_solver,
                           solver, square, strict, u_bar_rel, whole_run, write_pgm)
from tests.reference import HOLD, REPEAT, oracle_run, sched_index
from tests.test_gpu_inlet_profile import CONST_CASES, shear, wavy

pytestmark = pytest.mark.gpu


# ---- 1. the schedule [1.0] is no schedule, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("plan,precision,mask", CONST_CASES, ids=["-".join(str(v) for v in c) for c in CONST_CASES])
def test_the_schedule_of_ones_is_no_schedule(lbm, plan, precision, mask):
    nx, ny, steps, of = 1000, 200, 23, 7       # (1000 % 64 != 0: ragged last tiles)
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.08, precision=precision)
    opts = TALL_F32 if plan == "tall-f32" else PLANS["rowil-col5-nt"] if plan == "col5-f32" else PLANS[plan]
    solid = square(nx, ny) if mask else None
    a = run_ctx(lbm, nx, ny, opts, steps, of, solid=solid, **kw)
    b = run_ctx(lbm, nx, ny, opts, steps, of, solid=solid, inlet_schedule=[1.0], **kw)
    assert_same_results(a, b)
    # The schedule changes no launch, so a pinned plan names the same kernel. A measured plan (tune: "auto", "fast-auto") names the
    # kernel its own timing picked: the names are compared where both measurements picked the same plan.
    if (opts and opts.get("tune") == 0) or a.plan == b.plan:
        assert a.kernel_name == b.kernel_name, (a.kernel_name, b.kernel_name)


@pytest.mark.parametrize("plan", ["rowil-site-nt", "rowil-col5-nt", "planar-deep7-alt", "fast-rowil-col6"])
def test_a_constant_schedule_is_the_scaled_profile(lbm, plan):
    nx, ny, steps, of = 1000, 200, 23, 7
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.08)
    u = shear(ny, 0.05)
    a = run_ctx(lbm, nx, ny, PLANS[plan], steps, of, inlet_profile=0.7 * u, **kw)
    b = run_ctx(lbm, nx, ny, PLANS[plan], steps, of, inlet_profile=u, inlet_schedule=[0.7], **kw)
    assert_same_results(a, b)
    assert a.kernel_name == b.kernel_name


# ---- 2. schedules against the reference -------------------------------------------------------------------------------------------
def oracle_case(lbm, name, nx, ny):
    """(u or None, mask or None, s, mode). The pulse's period 7 is coprime to every launch depth 5..8, so a level that takes the wrong
    entry cannot cancel out; the ramp's clamp (t = 22) falls inside a fused launch; the third reverses the inflow."""
    if name == "pulse7":
        return None, None, lbm.sine_pulse(0.5, 7), REPEAT
    if name == "ramp22":
        return None, None, lbm.cosine_ramp(22), HOLD
    return lbm.parabolic_profile(ny, 0.05), masks(nx, ny)["inlet-outlet"], np.cos(2 * np.pi * np.arange(11) / 11), REPEAT


@pytest.mark.parametrize("name", ["pulse7", "ramp22", "reversing11"])
def test_schedules_against_the_reference(lbm, name):
    nx, ny, steps, of = 200, 64, 60, 20        # (200 % 64 != 0: a ragged last tile column)
    kw = dict(inlet_velocity=0.05)
    u, mask, s, mode = oracle_case(lbm, name, nx, ny)
    ref = oracle_run(nx, ny, steps, of, schedule=(s, mode), mask=mask, u=u, **kw)
    assert ref.first_unstable == -1
    if name == "reversing11":
        assert np.min(s) < 0
    uu = np.full(ny, 0.05) if u is None else u
    fluid0 = np.ones(ny, bool) if mask is None else mask[:, 0] == 0
    last = uu * s[sched_index(steps - 1, len(s), mode)]
    assert np.array_equal(ref.ux[fluid0, 0], last[fluid0])
    seen = {}
    for plan in ORACLE_PLANS:
        out = []
        for calls in ((steps,), (13, 29, 18)):       # one call; three calls: the iteration bookkeeping across calls, single-launch tails
            with lbm.Context(nx, ny, options=PLANS[plan], solid=mask, inlet_profile=u, inlet_schedule=(s, mode), **kw) as ctx:
                ctx.initialise()
                for n in calls:
                    ctx.step(n, of)
                assert ctx.first_unstable_step() == -1 and ctx.steps_done == steps
                out.append((ctx.populations("f_next"), ctx.drain_force_log(), ctx.macros()))
        fn, log, macros = out[0]
        assert np.array_equal(out[1][0], fn) and out[1][1] == log, plan
        for x, y in zip(out[1][2], macros):
            assert np.array_equal(x, y), plan
        assert np.array_equal(macros[1][fluid0, 0], last[fluid0]), plan       # the inlet column reports u[y] * s(steps - 1)
        key = "strict" if strict(plan) else "fast"
        seen.setdefault(key, fn)
        assert np.array_equal(fn, seen[key]), plan      # every plan of one arithmetic mode: the same bits
        assert_matches_reference(plan, fn, macros, log, ref, u_bar_rel(ref), fast_rho=False)     # (strict rho at 1e-14 too)


# ---- 3. the inlet column through every reporter ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-deep6-nt"])
def test_the_inlet_column_through_every_reporter(lbm, plan, precision):
    nx, ny = 200, 64
    T = np.float64 if precision == "f64" else np.float32
    kw = dict(inlet_velocity=0.05, precision=precision)
    u = shear(ny, 0.05)
    s = lbm.sine_pulse(0.5, 7)

    def column(t):          # (T)u[y] * (T)s(t): one multiplication in the element type
        return (u.astype(T) * T(s[t % 7])).astype(np.float64)
    with lbm.Context(nx, ny, options=PLANS[plan], inlet_profile=u, inlet_schedule=(s, "repeat"), **kw) as ctx:
        ctx.initialise()
        assert ctx.inlet_schedule_length() == 7
        for t in (0, 1, 6, 7, 8, 2 ** 31 - 1):
            assert ctx.inlet_scale(t) == float(T(s[t % 7]))
        rho0, ux0, uy0 = ctx.macros()          # the initial snapshot: ux = (T)(u[y] * s[0]), the product formed in double
        sol = ctx.solid().astype(bool)
        assert np.array_equal(ux0[~sol], np.broadcast_to((u * s[0]).astype(T).astype(np.float64)[:, None], (ny, nx))[~sol])
        done = 0
        for k in (1, 6, 7, 13):
            ctx.step(k - done, 0)
            done = k
            assert np.array_equal(ctx.macros()[1][:, 0], column(k - 1)), k
        # probes on the nodes (0, y), every iteration: sample t carries u[y] * s(t)
        ctx.probes_begin(np.stack([np.zeros(ny), np.arange(ny, dtype=np.float64)], axis=1))
        ctx.step(40, 1)
        ts, samples = ctx.drain_probes()
        assert list(ts) == list(range(13, 53))
        for t, smp in zip(ts, samples):
            assert np.array_equal(smp[:, 1], column(int(t))), t
        ctx.probes_end()
        # statistics: the sum of ux over the samples of column 0 is the host's sum of those products, in sample order
        ctx.stats_begin(0)
        ctx.step(21, 3)            # samples at t = 54, 57, ..., 72 (steps_done was 53)
        pts = [t for t in range(53, 74) if t % 3 == 0]
        assert ctx.stats_samples() == len(pts)
        acc = np.zeros(ny)
        for t in pts:
            acc = acc + column(t)
        assert np.array_equal(ctx.stats_sums()[1][:, 0], acc)


def test_without_a_schedule_the_scale_is_one(lbm):
    with lbm.Context(64, 32) as ctx:
        assert ctx.inlet_schedule_length() == 0 and ctx.inlet_scale(0) == 1.0 and ctx.inlet_scale(12345) == 1.0
        ctx.set_inlet_schedule([0.25, 0.5])
        assert ctx.inlet_schedule_length() == 2 and ctx.inlet_scale(5) == 0.5
        ctx.set_inlet_schedule([])
        assert ctx.inlet_schedule_length() == 0 and ctx.inlet_scale(5) == 1.0


# ---- 4. strips --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstrips", [3, 4])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd"])
@pytest.mark.parametrize("name", ["pulse13", "ramp50"])
def test_group_strips_with_a_schedule(lbm, name, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(inlet_velocity=0.06)
    u = wavy(ny, 0.06)
    sched = (lbm.sine_pulse(0.4, 13), "repeat") if name == "pulse13" else (lbm.cosine_ramp(50), "hold")
    w = whole_run(lbm, nx, ny, plan, steps, of, inlet_profile=u, inlet_schedule=sched, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], inlet_profile=u, inlet_schedule=sched, **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)


@pytest.mark.parametrize("plan", [None, "rowil-col5-nt"])
def test_host_staged_strips_with_a_schedule(lbm, plan):
    nx, ny = 512, 256
    kw = dict(inlet_velocity=0.05)
    u = wavy(ny, 0.05)
    sched = (lbm.sine_pulse(0.4, 13), "repeat")
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], inlet_profile=u, inlet_schedule=sched, **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, PLANS[plan] if plan else None, inlet_profile=u, inlet_schedule=sched, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


def test_a_scheduled_strip_replayed_from_a_graph(lbm):
    """One strip that is its own neighbour over the RCCL loopback (tests/test_gpu_thin_spots.py), issued eagerly and replayed from a
    hipGraph: the captured launches carry fixed iteration numbers and the graph advances the device word they count from, so every
    replay must take the schedule's next entries. The period 23 is coprime to the iterations of four launch groups (4 x 5 .. 8)."""
    nx, ny, steps, of = 512, 256, 437, 150
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    sched = (lbm.sine_pulse(0.4, 23), "repeat")
    base = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, loopback=2, deep_halo=2, overlap=1)
    out = []
    for graph in (0, 1):
        with lbm.Context(nx, ny, options=dict(base, graph=graph), inlet_schedule=sched, **kw) as ctx:
            ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            ctx.step(steps, of)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
            assert (ctx.graph_replays() > 0) == (graph == 1), (graph, ctx.graph_replays(), ctx.strip_schedule())
            out.append((ctx.populations("f_next")[1:-1], ctx.drain_force_log()))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


# ---- 5. fp32 ----------------------------------------------------------------------------------------------------------------------
def test_fp32_pulsed_run_against_fp64(lbm):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05)
    sched = (lbm.sine_pulse(0.3, 200), "repeat")
    with lbm.Context(nx, ny, inlet_schedule=sched, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", inlet_schedule=sched, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("inlet_schedule_fp32_vs_fp64", err_rho=er, err_u=eu)
    print("inlet_schedule_fp32_vs_fp64", er, eu)
    # the fp32 bars of tests/test_gpu_parity.py (rho 2e-5, u 2e-4; a uniform frozen inlet measures 1.2e-5 / 9.2e-5 there)
    assert er < 2e-5 and eu < 2e-4, (er, eu)
    want = np.float32(0.05) * np.float32(sched[0][(steps - 1) % 200])
    assert np.array_equal(m[1][:, 0], np.full(ny, float(want)))


# ---- 6. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_scheduled_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.07)
    s = lbm.cosine_ramp(200)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], inlet_schedule=s, **kw) as a:
        a.initialise()
        a.step(137, 0)                          # in mid-ramp
        a.save_state(tmp_path / "s.ckpt")
        a.step(100, 50)
        ref = (a.populations("f_next"), a.drain_force_log())
    data = open(tmp_path / "s.ckpt", "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word (bit 5), then the schedule's digest
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q", data[72:80]) == (32,)
    assert len(data) == 88 + 9 * nx * ny * 8
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], inlet_schedule=s, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "s.ckpt")
        assert b.steps_done == 137
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:        # a context that never saw the setter
        c.initialise()
        with pytest.raises(lbm.LbmError, match="with an inlet schedule; this context has none"):
            c.load_state(tmp_path / "s.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "plain.ckpt")
    with lbm.Context(nx, ny, inlet_schedule=s, **kw) as d:      # ... and one whose schedule was cleared again: the same bytes
        d.set_inlet_schedule([])
        d.initialise()
        d.step(3, 0)
        d.save_state(tmp_path / "cleared.ckpt")
    plain = open(tmp_path / "plain.ckpt", "rb").read()
    assert plain == open(tmp_path / "cleared.ckpt", "rb").read()
    assert plain[:8] == b"LBMCKPT1" and len(plain) == 72 + 9 * nx * ny * 8       # today's format: header, populations
    other = s.copy()
    other[5] += 1e-12
    with lbm.Context(nx, ny, inlet_schedule=other, **kw) as e:
        e.initialise()
        with pytest.raises(lbm.LbmError, match="different inlet schedule"):
            e.load_state(tmp_path / "s.ckpt")
        with pytest.raises(lbm.LbmError, match="without an inlet schedule; this context has one"):
            e.load_state(tmp_path / "plain.ckpt")
    with lbm.Context(nx, ny, inlet_schedule=(s, "repeat"), **kw) as f:      # the mode is part of the schedule
        f.initialise()
        with pytest.raises(lbm.LbmError, match="different inlet schedule"):
            f.load_state(tmp_path / "s.ckpt")
    # with a mask and a profile: flag bits 0, 1 and 5, three digests
    mask, u = square(nx, ny), lbm.parabolic_profile(ny, 0.07)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, inlet_schedule=s, **kw) as g:
        g.initialise()
        g.step(11, 0)
        g.save_state(tmp_path / "all.ckpt")
        g.load_state(tmp_path / "all.ckpt")
    head = open(tmp_path / "all.ckpt", "rb").read(104)
    assert head[:8] == b"LBMCKPT3" and struct.unpack("<Q", head[72:80]) == (1 | 2 | 32,)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, **kw) as h:
        h.initialise()
        with pytest.raises(lbm.LbmError, match="with an inlet schedule; this context has none"):
            h.load_state(tmp_path / "all.ckpt")


# ---- 7. arguments -----------------------------------------------------------------------------------------------------------------
def test_set_inlet_schedule_arguments(lbm):
    nx, ny = 128, 32
    dp = C.POINTER(C.c_double)
    with lbm.Context(nx, ny, inlet_velocity=0.05) as ctx:
        L = ctx.L

        def call(arr, n, mode=0):
            a = np.ascontiguousarray(arr, dtype=np.float64)
            return L.lbm_set_inlet_schedule(ctx.h, a.ctypes.data_as(dp), n, mode)
        s = lbm.cosine_ramp(10)
        assert L.lbm_set_inlet_schedule(ctx.h, None, 3, 0) == -1 and b"null table" in L.lbm_last_error()
        assert call(s, -1) == -1 and b"n = -1" in L.lbm_last_error()
        assert call(s, 1048577) == -1 and b"n = 1048577" in L.lbm_last_error()
        assert call(s, 11, 2) == -1 and b"mode = 2" in L.lbm_last_error()
        assert call(s, 11, -1) == -1 and b"mode = -1" in L.lbm_last_error()
        for bad in (np.nan, np.inf, -np.inf):
            b = s.copy(); b[7] = bad
            assert call(b, 11) == -1 and b"entry 7" in L.lbm_last_error()
        assert ctx.inlet_schedule_length() == 0
        assert call(s, 11, 1) == 0 and ctx.inlet_schedule_length() == 11
        assert L.lbm_set_inlet_schedule(ctx.h, None, 0, 0) == 0 and ctx.inlet_schedule_length() == 0       # n == 0 clears
        assert call(s, 11) == 0
        v = C.c_double()
        assert L.lbm_get_inlet_scale(ctx.h, -1, C.byref(v)) == -1 and b"t = -1" in L.lbm_last_error()
        assert L.lbm_get_inlet_scale(ctx.h, 3, None) == -1 and b"null" in L.lbm_last_error()
        ctx.initialise()
        assert call(s, 11) == -1 and b"before lbm_initialise" in L.lbm_last_error()
    # lbm_initialise knows profile and schedule: u[y] * s[k] must stay below 1, in either order of the two setters
    u = np.full(ny, 0.05)
    u[9] = 0.4
    for first in ("profile", "schedule"):
        with lbm.Context(nx, ny, inlet_velocity=0.05) as ctx:
            if first == "profile":
                ctx.set_inlet_profile(u)
            ctx.set_inlet_schedule([1.0, 2.0, 2.5, 1.0])
            if first == "schedule":
                ctx.set_inlet_profile(u)
            with pytest.raises(lbm.LbmError, match=r"row 9 .*entry 2 "):
                ctx.initialise()
    with lbm.Context(nx, ny, inlet_velocity=0.05) as ctx:      # negative products are allowed, and so is anything below 1
        ctx.set_inlet_profile(u)
        ctx.set_inlet_schedule([1.0, 2.0, 2.4999, -30.0])
        ctx.initialise()
        ctx.step(2, 0)
    with pytest.raises(ValueError):
        lbm.Context(nx, ny, inlet_schedule=([1.0], "sometimes"))


# ---- 8. the host CLI --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
@pytest.mark.parametrize("source", ["file", "pulse"])
def test_lbm_solver_inlet_schedule_matches_the_binding(lbm, solver, tmp_path, source, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    mean = 0.04
    mask = np.zeros((ny, nx), np.uint8)
    mask[18:30, 30:42] = 1                    # square, frontal height D = 12
    write_pgm(tmp_path / "sq.pgm", mask * 255)
    if source == "file":
        s = 0.2 + 0.8 * lbm.cosine_ramp(120)
        (tmp_path / "sched.txt").write_text("# a ramp from 0.2\n" + "\n".join(repr(float(v)) for v in s) + "\n")
        args, sched, spec = ["--inlet-schedule", str(tmp_path / "sched.txt")], (s, "hold"), str(tmp_path / "sched.txt")
    else:
        args, sched, spec = ["--inlet-pulse", "0.3:50"], (lbm.sine_pulse(0.3, 50), "repeat"), "pulse:0.3:50"
        # (the C++ builder and the helper may differ in the last bit of sin: the schedule the solver used is the one it prints)
        pr = run_solver(args + ["--print-inlet-schedule"], tmp_path)
        sched = (np.array([float(l) for l in pr.stdout.split()]), "repeat")
        assert np.max(np.abs(sched[0] - lbm.sine_pulse(0.3, 50))) <= 4e-16
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--inlet-velocity", str(mean),
                     "--no-vtk", "--obstacle-mask", str(tmp_path / "sq.pgm")] + args + extra, tmp_path)
    assert "Inlet: schedule " + spec in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, inlet_velocity=mean, solid=mask, inlet_schedule=sched) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.first_unstable_step() == -1
        log = ctx.drain_force_log()
        rho, ux, uy = ctx.macros()
        last = mean * ctx.inlet_scale(steps - 1)
    q = 0.5 * mean * mean * 12                # Cd / Cl keep referring to the inlet velocity
    assert [int(r[0]) for r in rows] == [t for t, _, _ in log]
    for r, (t, fx, fy) in zip(rows, log):
        for got, want in zip(map(float, r[1:]), (fx, fy, fx / q, fy / q)):
            assert abs(got - want) <= 1.5e-8, (t, r)
    cux, cuy, crho = read_velocity_field(tmp_path / "velocity_field.csv", nx, ny)
    assert np.max(np.abs(cux[:, 0] - last)) <= 5.1e-9           # the inlet column is the scaled inflow (8 decimals)
    for got, want in ((cux, ux), (cuy, uy), (crho, rho)):
        assert np.max(np.abs(got - want)) <= 5.1e-9
    params = read_params(tmp_path / "simulation_params.csv")
    assert params["inlet_schedule"] == spec and params["obstacle_mask"].endswith("sq.pgm")
    keys = list(params)
    assert keys.index("inlet_schedule") == len(keys) - 1
