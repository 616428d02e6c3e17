"""Free-slip and moving top / bottom walls (lbm_set_wall, Context/Group(walls=...), lbm_solver --wall-south / --wall-north / --walls) on the GPU.

The reference is oracle_run(walls=...) of tests/reference.py: the stepwise oracle loop, whose boundary step is a numpy restatement of all
of lbmo_boundaries, the two walls with their kind and k = u_w / 6 first. fp64, IEEE, in the operation order of the library's strict
arithmetic: strict plans must match it bit for bit, contracted ones within 1e-10 (the bars of the TRT and LES tests).
tests/test_reference_cpu.py pins the loop, with two no-slip walls, to the unmodified oracle."""
import functools
import importlib
import struct

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PKG, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, host_staged_two_strips,  # noqa: F401
                           lbm_gpu, read_csv_rows, read_params, read_velocity_field, record, run_solver, square, whole_run)
from tests.reference import FREESLIP, NOSLIP, REPEAT, moving, oracle_run, trt_collide

pytestmark = pytest.mark.gpu


# ---- 1. every plan against the reference ----------------------------------------------------------------------------------------
NX, NY, STEPS, OF = 160, 48, 240, 60
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
# name -> (walls, the square mask and the parabolic inlet too?)
CASES = {
    "free-free": ((FREESLIP, FREESLIP), False),
    "free-noslip": ((FREESLIP, NOSLIP), False),
    "moving-moving": ((moving(0.08), moving(0.08)), False),
    "noslip-moving": ((NOSLIP, moving(0.05)), False),
    "moving-free": ((moving(-0.03), FREESLIP), False),
    "moving-free-square-parabolic": ((moving(-0.03), FREESLIP), True),
}
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))


def case_inputs(name, lbm):
    walls, extras = CASES[name]
    mask = square(NX, NY) if extras else None
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"]) if extras else None
    return walls, mask, u


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the reference run of the case, max |f_next - f_next of the same case between two no-slip walls|); on the CPU, once."""
    lbm = importlib.import_module(PKG)
    walls, mask, u = case_inputs(name, lbm)
    ref = oracle_run(NX, NY, STEPS, OF, walls=walls, mask=mask, u=u, **KW)
    plain = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, **KW)
    return ref, float(np.max(np.abs(ref.f_next - plain.f_next)))


@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("name", list(CASES))
def test_walls_against_the_reference(lbm, name, plan):
    for other in CASES:                               # precondition, on the CPU before any GPU run: stable, and not two no-slip walls
        ref_o, away = reference(other)
        assert ref_o.first_unstable == -1, other
        assert away > 1e-3, (other, away)             # the walls are active: the test cannot pass with them ignored
    walls, mask, u = case_inputs(name, lbm)
    ref, _ = reference(name)
    with lbm.Context(NX, NY, options=PLANS[plan], solid=mask, inlet_profile=u, walls=walls, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 1b. a second collision operator under the walls: TRT against the reference loop with trt_collide -----------------------------
TRT_MAGIC, TRT_WALLS = 3.0 / 16.0, (moving(0.05), FREESLIP)


@functools.lru_cache(maxsize=None)
def trt_reference():
    ref = oracle_run(NX, NY, STEPS, OF, walls=TRT_WALLS, collide=functools.partial(trt_collide, magic=TRT_MAGIC), **KW)
    plain = oracle_run(NX, NY, STEPS, OF, collide=functools.partial(trt_collide, magic=TRT_MAGIC), **KW)
    return ref, float(np.max(np.abs(ref.f_next - plain.f_next)))


@pytest.mark.parametrize("plan", ORACLE_PLANS)
def test_trt_with_walls_against_the_reference(lbm, plan):
    ref, away = trt_reference()
    assert ref.first_unstable == -1 and away > 1e-3, away          # on the CPU, before the GPU run: stable, and the walls are active
    with lbm.Context(NX, NY, options=PLANS[plan], trt_magic=TRT_MAGIC, walls=TRT_WALLS, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == -1 and ctx.kernel_name().endswith((",4>", ",5>"))
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 1c. every feature of the boundary step at once: an inlet schedule on a profile, TRT, both walls, a mask -------------------------
@functools.lru_cache(maxsize=None)
def cross_reference():
    """(the reference run, [max |f_next - f_next of the same case with one feature switched off|: walls, schedule, TRT]); on the CPU,
    once. The pulse's period 7 is coprime to every launch depth."""
    lbm = importlib.import_module(PKG)
    on = dict(mask=square(NX, NY), u=lbm.parabolic_profile(NY, KW["inlet_velocity"]), walls=TRT_WALLS,
              schedule=(lbm.sine_pulse(0.3, 7), REPEAT), collide=functools.partial(trt_collide, magic=TRT_MAGIC))
    ref = oracle_run(NX, NY, STEPS, OF, **on, **KW)
    away = [float(np.max(np.abs(ref.f_next - oracle_run(NX, NY, STEPS, OF, **dict(on, **off), **KW).f_next)))
            for off in (dict(walls=NOSLIP), dict(schedule=None), dict(collide=None))]
    return ref, on, away


@pytest.mark.parametrize("plan", ORACLE_PLANS)
def test_schedule_with_trt_and_walls_against_the_reference(lbm, plan):
    ref, on, away = cross_reference()
    assert ref.first_unstable == -1 and min(away) > 1e-3, away     # on the CPU, before the GPU run: stable, and each feature is active
    with lbm.Context(NX, NY, options=PLANS[plan], solid=on["mask"], inlet_profile=on["u"], inlet_schedule=(on["schedule"][0], "repeat"),
                     trt_magic=TRT_MAGIC, walls=TRT_WALLS, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == -1 and ctx.kernel_name().endswith((",4>", ",5>"))
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 2. free-slip keeps a uniform stream uniform ----------------------------------------------------------------------------------
def uniformity(rho, ux, uy, u0):
    return float(np.max(np.abs(ux - u0))), float(np.max(np.abs(uy))), float(np.max(np.abs(rho - 1.0)))


def test_free_slip_keeps_a_uniform_stream_uniform(lbm):
    nx, ny, steps, u0 = 160, 48, 600, 0.08
    kw = dict(tau=0.55, inlet_velocity=u0)
    empty = np.zeros((ny, nx), np.uint8)
    plain = oracle_run(nx, ny, steps, 0, mask=empty, **kw)          # precondition, on the CPU: no-slip walls do disturb the stream
    assert plain.first_unstable == -1 and max(uniformity(plain.rho, plain.ux, plain.uy, u0)) > 1e-2
    ref = oracle_run(nx, ny, steps, 0, walls=FREESLIP, mask=empty, **kw)
    record("walls_uniform_stream_reference", err=uniformity(ref.rho, ref.ux, ref.uy, u0))
    with lbm.Context(nx, ny, solid=empty, walls="free-slip", options=dict(arith=0), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        eu, ev, er = uniformity(*ctx.macros(), u0)
    record("walls_uniform_stream_gpu", err=(eu, ev, er))
    assert eu <= 1e-12 and ev <= 1e-12 and er <= 1e-12, (eu, ev, er)


# ---- 3. no-slip is today's code -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col5-nt", "planar-fuse3-8", "fast-rowil-col6", "rowil-deep6-nt", "planar-site"])
def test_two_no_slip_walls_are_the_default(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in ({}, dict(walls=None), dict(walls=(NOSLIP, NOSLIP))):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.populations("f_current")))
    with lbm.Context(nx, ny, options=PLANS[plan], walls=(moving(0.05), FREESLIP), **kw) as ctx:     # set, then cleared
        ctx.set_wall("south", "no-slip")
        ctx.set_wall("north", "no-slip")
        assert ctx.walls() == ((NOSLIP, 0.0), (NOSLIP, 0.0))
        ctx.initialise()
        ctx.step(steps, of)
        out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.populations("f_current")))
    a = out[0]
    for b in out[1:]:
        assert a[0] == b[0]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4]) and a[3] == b[3]
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y)


# ---- 4. strips ------------------------------------------------------------------------------------------------------------------
STRIP_WALLS = (moving(0.05), FREESLIP)


@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_context_with_walls(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1, walls=STRIP_WALLS)
    w = whole_run(lbm, nx, ny, plan, steps, of, **kw)
    plain = whole_run(lbm, nx, ny, plan, steps, of, tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
    assert float(np.max(np.abs(w[1] - plain[1]))) > 1e-3          # the walls are active in the run the strips are held to
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert [c.walls() for c in g.ctxs] == [(("moving", 0.05), (FREESLIP, 0.0))] * nstrips
        assert_group_is_whole(g, w)


def test_host_staged_strips_with_walls(lbm):
    nx, ny = 512, 256
    kw = dict(tau=0.55, inlet_velocity=0.08, walls=STRIP_WALLS)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, None, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 5. stability follows the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [NOSLIP, FREESLIP])
def test_stability_follows_the_reference(lbm, walls):
    stab = dict(tau=0.505, inlet_velocity=0.1)
    want = oracle_run(400, 100, 4000, 0, walls=walls, **stab).first_unstable
    with lbm.Context(400, 100, options=dict(arith=0), walls=(walls, walls), **stab) as ctx:
        ctx.initialise()
        ctx.step(4000, 0)
        got = ctx.first_unstable_step()
    record("walls_stability_%s" % walls, reference_first_unstable=want, gpu_first_unstable=got)
    assert want >= 0 and got == want


# ---- 6. fp32 against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_free_slip_against_fp64(lbm, arith):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05, walls="free-slip")     # tau: the default, 0.6, as in test_gpu_parity.py's fp32 comparison
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=dict(arith=arith), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("walls_fp32_vs_fp64_arith%d" % arith, err_rho=er, err_u=eu)
    assert er < 2e-5 and eu < 2e-4, (er, eu)     # the fp32 bars of tests/test_gpu_parity.py


# ---- 7. the reporting layers ride along -------------------------------------------------------------------------------------------
REPORT_KW = dict(tau=0.55, inlet_velocity=0.06, walls=(moving(0.05), FREESLIP))


@functools.lru_cache(maxsize=None)
def twin_macros(nx, ny, steps):
    """macros() of a plain run of `steps` steps under REPORT_KW: what a sample of iteration steps - 1 must equal."""
    lbm = importlib.import_module(PKG)
    with lbm.Context(nx, ny, **REPORT_KW) as twin:
        twin.initialise()
        twin.step(steps, 0)
        return twin.macros()


def test_statistics_sample_equals_macros_one_step_later_with_walls(lbm):
    nx, ny = 128, 48
    with lbm.Context(nx, ny, **REPORT_KW) as ctx:
        ctx.initialise()
        ctx.stats_begin(40)
        ctx.step(41, 40)                   # one sample, at t = 40
        assert ctx.stats_samples() == 1
        sums = ctx.stats_sums()
    rho, ux, uy = twin_macros(nx, ny, 41)
    for got, want in zip(sums, (rho, ux, uy, ux * ux, uy * uy, ux * uy)):
        assert np.array_equal(got, want)


def test_probes_on_the_wall_rows_equal_the_macros_with_walls(lbm):
    nx, ny = 128, 48
    pts = [(0, 0), (37, 0), (nx - 1, 0), (0, ny - 1), (90, ny - 1), (nx - 1, ny - 1)]     # nodes of row 0 and of row ny - 1, corners included
    with lbm.Context(nx, ny, probes=np.array(pts, dtype=np.float64), **REPORT_KW) as ctx:
        ctx.initialise()
        ctx.step(41, 40)
        ts, vals = ctx.drain_probes()
    assert list(ts) == [0, 40]
    rho, ux, uy = twin_macros(nx, ny, 41)
    for j, (x, y) in enumerate(pts):
        assert np.array_equal(vals[1, j], np.array([rho[y, x], ux[y, x], uy[y, x]])), (x, y)


def test_fine_frame_equals_the_macros_rounded_to_float_with_walls(lbm):
    nx, ny = 128, 48
    with lbm.Context(nx, ny, frames=1, **REPORT_KW) as ctx:
        ctx.initialise()
        ctx.step(41, 40)
        frames = ctx.drain_frames()
    assert [t for t, _ in frames] == [0, 40]
    for got, want in zip(frames[1][1][:3], twin_macros(nx, ny, 41)):
        assert np.array_equal(got, want.astype(np.float32))


# ---- 8. checkpoints -----------------------------------------------------------------------------------------------------------------
def test_walls_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(tau=0.55, inlet_velocity=0.07)
    walls = (moving(0.05), FREESLIP)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], walls=walls, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "walls.ckpt")
        a.step(100, 50)
        assert a.first_unstable_step() == -1
        ref = (a.populations("f_next"), a.drain_force_log())
    data = open(tmp_path / "walls.ckpt", "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word (bit 4), then (no digests, no collision
    # parameter) the four doubles south kind, south velocity, north kind, north velocity
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q4d", data[72:112]) == (16, 2.0, 0.05, 1.0, 0.0)
    assert len(data) == 112 + 9 * nx * ny * 8
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], walls=walls, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "walls.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:                                   # a default context: refuses the walls file, writes LBMCKPT1
        c.initialise()
        with pytest.raises(lbm.LbmError, match="wall"):
            c.load_state(tmp_path / "walls.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "plain.ckpt")
    plain = open(tmp_path / "plain.ckpt", "rb").read()
    assert plain[:8] == b"LBMCKPT1" and len(plain) == 72 + 9 * nx * ny * 8
    for other in ((moving(0.05), NOSLIP), (moving(0.06), FREESLIP), (FREESLIP, moving(0.05)), "free-slip"):
        with lbm.Context(nx, ny, walls=other, **kw) as d:
            d.initialise()
            with pytest.raises(lbm.LbmError, match="wall"):
                d.load_state(tmp_path / "walls.ckpt")
            with pytest.raises(lbm.LbmError, match="wall"):
                d.load_state(tmp_path / "plain.ckpt")
    u = lbm.parabolic_profile(ny, 0.07)
    mask = square(nx, ny)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, trt_magic=0.1875, walls=walls, **kw) as e:   # mask + profile + TRT + walls
        e.initialise()
        e.step(11, 0)
        e.save_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        want = e.populations("f_next")
        e.load_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        assert np.array_equal(e.populations("f_next"), want)
        with pytest.raises(lbm.LbmError):
            e.load_state(tmp_path / "walls.ckpt")
    head = open(tmp_path / "all.ckpt", "rb").read(72 + 8 + 8 + 8 + 8 + 32)
    assert head[:8] == b"LBMCKPT3" and struct.unpack("<Q", head[72:80]) == (1 | 2 | 8 | 16,)
    assert struct.unpack("<d4d", head[96:136]) == (0.1875, 2.0, 0.05, 1.0, 0.0)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, trt_magic=0.1875, **kw) as f:                # ... does not load without the walls
        f.initialise()
        with pytest.raises(lbm.LbmError, match="wall"):
            f.load_state(tmp_path / "all.ckpt")


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------
def test_set_wall_arguments(lbm):
    import ctypes as C
    with lbm.Context(128, 32) as ctx:
        L = ctx.L
        k, u = C.c_int(-7), C.c_double(-7.0)
        assert L.lbm_set_wall(None, 0, 1, 0.0) == -1 and b"null context" in L.lbm_last_error()
        assert L.lbm_get_wall(None, 0, C.byref(k), C.byref(u)) == -1 and b"null context" in L.lbm_last_error()
        assert ctx.walls() == ((NOSLIP, 0.0), (NOSLIP, 0.0))
        for side in (-1, 2, 7):
            assert L.lbm_set_wall(ctx.h, side, 1, 0.0) == -1 and b"side" in L.lbm_last_error()
            assert L.lbm_get_wall(ctx.h, side, C.byref(k), C.byref(u)) == -1 and b"side" in L.lbm_last_error()
        for kind in (-1, 3, 16):
            assert L.lbm_set_wall(ctx.h, 0, kind, 0.0) == -1 and b"kind" in L.lbm_last_error()
        for bad in (float("nan"), float("inf"), -float("inf"), 1.0, -1.0, 1.5):
            assert L.lbm_set_wall(ctx.h, 1, 2, bad) == -1, bad
            assert b"velocity" in L.lbm_last_error()
        for kind, name in ((0, b"no-slip"), (1, b"free-slip")):
            assert L.lbm_set_wall(ctx.h, 0, kind, 0.01) == -1 and b"velocity" in L.lbm_last_error() and name in L.lbm_last_error()
        assert ctx.walls() == ((NOSLIP, 0.0), (NOSLIP, 0.0))              # nothing of the refused calls stuck
        ctx.set_wall("south", "moving", -0.25)
        ctx.set_wall("north", "free-slip")
        assert ctx.walls() == (("moving", -0.25), (FREESLIP, 0.0))
        assert L.lbm_get_wall(ctx.h, 0, None, None) == 0                   # both pointers are nullable
        assert L.lbm_get_wall(ctx.h, 0, C.byref(k), None) == 0 and k.value == 2
        assert L.lbm_get_wall(ctx.h, 0, None, C.byref(u)) == 0 and u.value == -0.25
        ctx.set_wall("south", "no-slip")                                   # kind 0 clears a wall, velocity included
        assert ctx.get_wall("south") == (NOSLIP, 0.0) and ctx.get_wall("north") == (FREESLIP, 0.0)
        ctx.set_wall(0, 2, 0.999)
        ctx.initialise()
        assert L.lbm_set_wall(ctx.h, 0, 0, 0.0) == -1 and b"before lbm_initialise" in L.lbm_last_error()
        assert ctx.get_wall("south") == ("moving", 0.999)
    with pytest.raises(lbm.LbmError):
        lbm.Context(128, 32, walls=(("moving", 2.0), NOSLIP))
    with pytest.raises(ValueError):
        lbm.Context(128, 32, walls="sticky")
    with pytest.raises(ValueError):
        lbm.Context(128, 32, walls="moving")


# ---- 10. the host CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
@pytest.mark.parametrize("name", ["free-slip", "north-moving"])
def test_lbm_solver_walls_match_the_binding(lbm, tmp_path, name, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    tau, u0 = 0.55, 0.08
    args, walls, line, rows_want = {
        "free-slip": (["--walls", "free-slip"], "free-slip", "  Walls: south free-slip, north free-slip", ("free-slip", "free-slip")),
        "north-moving": (["--wall-north", "moving:0.05"], (NOSLIP, moving(0.05)), "  Walls: south no-slip, north moving u = 0.05",
                         ("no-slip", "moving:0.05")),
    }[name]
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--tau", str(tau),
                     "--inlet-velocity", str(u0), "--cylinder-radius", "0.1", "--no-vtk"] + args + extra, tmp_path)
    assert line in pr.stdout.splitlines(), pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=u0, cylinder_radius=0.1, walls=walls) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.first_unstable_step() == -1
        log = ctx.drain_force_log()
        rho, ux, uy = ctx.macros()
    assert [int(r[0]) for r in rows] == [t for t, _, _ in log]
    for r, (t, fx, fy) in zip(rows, log):
        for got, want in zip(map(float, r[1:3]), (fx, fy)):
            assert abs(got - want) <= 1.5e-8, (t, r)
    cux, cuy, crho = read_velocity_field(tmp_path / "velocity_field.csv", nx, ny)
    for got, want in ((cux, ux), (cuy, uy), (crho, rho)):
        assert np.max(np.abs(got - want)) <= 5.1e-9
    params = read_params(tmp_path / "simulation_params.csv")
    assert (params["wall_south"], params["wall_north"]) == rows_want
    assert abs(float(params["tau"]) - tau) < 1e-12


def test_lbm_solver_without_wall_options_says_nothing_about_walls(lbm, tmp_path):
    pr = run_solver(["--nx", "64", "--ny", "32", "--steps", "11", "--output-frequency", "5", "--no-vtk", "--walls", "no-slip"], tmp_path)
    assert "Walls:" not in pr.stdout
    assert not any(k.startswith("wall_") for k in read_params(tmp_path / "simulation_params.csv"))
