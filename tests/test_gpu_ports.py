"""Pressure and velocity ports at the inlet and the outlet (lbm_set_port, Context/Group(ports=...), lbm_solver --inlet / --outlet) on the GPU.

Every kernel family against tests/ports_reference.py (the reference loop with the table of include/lbm_hip.h in numpy): strict plans
f_next bit for bit, contracted plans within 1e-10, the bars of helpers.assert_matches_reference with U_BAR_ABS; the region edges of the
register kernel, the collision models, fp32 against single iterations, strips against the whole domain, the snapshot's consumers,
checkpoints, the defaults, a pressure-driven channel, the arguments and the command line. Every test needs lbm_set_port."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from tests import feature_cases as fc
from tests.forcing_reference import guo_collide
from tests.helpers import (ORACLE_PLANS, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, lbm_gpu, read_params,  # noqa: F401
                           read_velocity_field, run_solver, strict, whole_run)
from tests.ports_reference import CHANNEL, PRESSURE, VELOCITY, channel_run, ports_run
from tests.reference import FREESLIP, les_collide, moving, oracle_run, trt_collide

pytestmark = pytest.mark.gpu

NX, NY, STEPS, OF = 130, 70, 23, 8            # three deep launches and a remainder at every depth; the last 64-wide region holds two columns
WALLS = (FREESLIP, moving(0.05))
KW = dict(tau=0.6, inlet_velocity=0.05)
PAIRS = {
    "velocity-pressure0.985": (VELOCITY, (PRESSURE, 0.985)),
    "pressure1.02-pressure1": ((PRESSURE, 1.02), (PRESSURE, 1.0)),
    "pressure1.015-velocity0.03": ((PRESSURE, 1.015), (VELOCITY, 0.03)),
    "velocity-velocity0.04": (VELOCITY, (VELOCITY, 0.04)),
}
FAMILY_PLANS = ORACLE_PLANS + ["park10", "park11"]


def read_only(run):
    for a in (run.f_next, run.rho, run.ux, run.uy):
        a.flags.writeable = False
    return run


def run_plan(lbm, nx, ny, plan, steps, of, **kw):
    """(f_next, macros, force log, kernel name) of a context on a plan of helpers.PLANS or feature_cases.PINNED."""
    with lbm.Context(nx, ny, options=fc.plan_options(plan), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.first_unstable_step() == -1
        return ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.kernel_name()


# ---- 1. every kernel family, the four port pairs -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_reference(name):
    """(the reference run, max |f_next - f_next with the default ports|); on the CPU, once."""
    ref = ports_run(NX, NY, STEPS, OF, ports=PAIRS[name], walls=WALLS, **KW)
    plain = oracle_run(NX, NY, STEPS, OF, walls=WALLS, **KW)
    return read_only(ref), float(np.max(np.abs(ref.f_next - plain.f_next)))


@pytest.mark.parametrize("plan", FAMILY_PLANS)
@pytest.mark.parametrize("name", list(PAIRS))
def test_every_family_against_the_reference(lbm, name, plan):
    ref, away = pair_reference(name)
    assert ref.first_unstable == -1 and away > 1e-3, away            # on the CPU, before the GPU run: stable, and the ports are active
    fn, macros, log, _ = run_plan(lbm, NX, NY, plan, STEPS, OF, ports=PAIRS[name], walls=WALLS, **KW)
    assert_matches_reference(fc.contracted(plan), fn, macros, log, ref, U_BAR_ABS)


# ---- 2. region edges: the east port's column alone in its region, solid cells in both port columns and two corners --------------------
EDGE_PAIRS = [((PRESSURE, 1.015), (VELOCITY, 0.03)), (VELOCITY, (PRESSURE, 0.985))]


def edge_mask(nx, ny):
    m = np.zeros((ny, nx), np.uint8)
    m[0, 0] = m[ny - 1, nx - 1] = 1                                 # two corners
    m[ny // 3, 0] = m[ny // 2, 0] = 1                               # the west port's column
    m[ny // 4, nx - 1] = m[(2 * ny) // 3, nx - 1] = 1               # the east port's column
    m[ny // 2, nx // 2] = 1
    return m


@functools.lru_cache(maxsize=None)
def edge_reference(nx, ny, k, steps):
    mask = edge_mask(nx, ny) if nx > 3 else np.zeros((ny, nx), np.uint8)
    return read_only(ports_run(nx, ny, steps, OF, ports=EDGE_PAIRS[k], mask=mask, walls=WALLS, **KW)), mask


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("nx, ny", [(65, 25), (64, 24), (129, 41)])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "planar-col6-alt", "fast-rowil-col6", "fast-planar-col5"])
def test_region_edges(lbm, plan, nx, ny, k):
    ref, mask = edge_reference(nx, ny, k, STEPS)
    assert ref.first_unstable == -1
    fn, macros, log, name = run_plan(lbm, nx, ny, plan, STEPS, OF, ports=EDGE_PAIRS[k], solid=mask, walls=WALLS, **KW)
    assert name.startswith("k_stepc_col<double")
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("nx, ny", [(2, 2), (3, 2)])
def test_smallest_lattices(lbm, nx, ny, k):
    ref, mask = edge_reference(nx, ny, k, 7)
    assert ref.first_unstable == -1
    fn, macros, log, _ = run_plan(lbm, nx, ny, "rowil-site-nt", 7, OF, ports=EDGE_PAIRS[k], solid=mask, walls=WALLS, **KW)
    assert_matches_reference("rowil-site-nt", fn, macros, log, ref, U_BAR_ABS)


# ---- 3. the collision models -----------------------------------------------------------------------------------------------------------
MODEL_PORTS = ((PRESSURE, 1.01), (PRESSURE, 0.99))
MODELS = {
    "les": (dict(smagorinsky=0.17), functools.partial(les_collide, cs=0.17), 0.52, (",2>", ",3>")),
    "trt": (dict(trt_magic=3.0 / 16.0), functools.partial(trt_collide, magic=3.0 / 16.0), 0.6, (",4>", ",5>")),
    "forced": (dict(forcing=(2e-5, -1e-5)), functools.partial(guo_collide, force=(2e-5, -1e-5)), 0.6, (",8>", ",9>")),
}


@functools.lru_cache(maxsize=None)
def model_reference(model):
    _, collide, tau, _ = MODELS[model]
    return read_only(ports_run(NX, NY, STEPS, OF, ports=MODEL_PORTS, walls=WALLS, collide=collide, tau=tau, inlet_velocity=0.05))


@pytest.mark.parametrize("plan", ["rowil-col5-nt", "fast-rowil-col6", "rowil-deep6-nt", "planar-fuse3-8"])
@pytest.mark.parametrize("model", list(MODELS))
def test_collision_models_with_ports(lbm, model, plan):
    ckw, _, tau, suffix = MODELS[model]
    ref = model_reference(model)
    assert ref.first_unstable == -1
    fn, macros, log, name = run_plan(lbm, NX, NY, plan, STEPS, OF, ports=MODEL_PORTS, walls=WALLS, tau=tau, inlet_velocity=0.05, **ckw)
    assert name.endswith(suffix), name
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 4. fp32: every plan of an arithmetic mode is that mode's site plan; both stay at the fp32 bars of the fp64 reference ---------------
F32_PORTS = ((PRESSURE, 1.015), (VELOCITY, 0.03))
F32_NX, F32_NY = 130, 100                      # (the tall regions are 48 rows high)
F32_PLANS = {0: ["rowil-col5-nt", "planar-col6-alt", "rowil-col7-alt", "rowil-deep6-nt", "planar-fuse3-8", "tall-f32"],
             1: ["fast-rowil-col6", "fast-planar-col5", "fast-rowil-col7", "fast-rowil-deep7", "tall-f32-fast"]}
ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)


@functools.lru_cache(maxsize=None)
def f32_site(lbm, arith):
    with lbm.Context(F32_NX, F32_NY, precision="f32", options=dict(ONE, arith=arith), ports=F32_PORTS, walls=WALLS, **KW) as one:
        one.initialise()
        one.step(STEPS, OF)
        assert one.kernel_name().startswith("k_step_site<float") and one.first_unstable_step() == -1
        return one.populations("f_next"), one.macros(), one.drain_force_log()


@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_plans_equal_the_site_plan_and_hold_the_fp32_bars(lbm, arith):
    ref = ports_run(F32_NX, F32_NY, STEPS, OF, ports=F32_PORTS, walls=WALLS, **KW)
    s_fn, s_macros, s_log = f32_site(lbm, arith)
    uscale = float(np.max(np.sqrt(ref.ux ** 2 + ref.uy ** 2)))
    er = float(np.max(np.abs(s_macros[0] - ref.rho)) / np.max(np.abs(ref.rho)))
    eu = max(float(np.max(np.abs(s_macros[1] - ref.ux))), float(np.max(np.abs(s_macros[2] - ref.uy)))) / uscale
    print("fp32 arith %d against the fp64 reference: rho %.3g, u %.3g" % (arith, er, eu))
    assert er < 2e-5 and eu < 2e-4, (er, eu)                         # the fp32 bars of tests/test_gpu_walls.py
    assert np.all(s_macros[0][:, 0] == float(np.float32(1.015))) and np.all(s_macros[1][:, -1] == float(np.float32(0.03)))   # the given ones, as cast
    for plan in F32_PLANS[arith]:
        with lbm.Context(F32_NX, F32_NY, precision="f32", options=fc.plan_options(plan), ports=F32_PORTS, walls=WALLS, **KW) as ctx:
            ctx.initialise()
            ctx.step(STEPS, OF)
            assert ctx.kernel_name().replace(" ", "").startswith(("k_stepc_col<float", "k_stepd_tile<float", "k_step3_tile<float")), (plan, ctx.kernel_name())
            assert np.array_equal(ctx.populations("f_next"), s_fn), plan
            for a, b in zip(ctx.macros(), s_macros):
                assert np.array_equal(a, b), plan
            assert ctx.drain_force_log() == s_log, plan             # (one force kernel on equal populations: equal rows)


# ---- 5. strips ------------------------------------------------------------------------------------------------------------------------
STRIP_PORTS = ((PRESSURE, 1.015), (VELOCITY, 0.03))


@pytest.mark.parametrize("nstrips", [2, 3, 4])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_context_with_ports(lbm, plan, nstrips):
    kw = dict(walls=WALLS, ports=STRIP_PORTS, **KW)
    w = whole_run(lbm, NX, NY, plan, STEPS, OF, **kw)
    plain = whole_run(lbm, NX, NY, plan, STEPS, OF, walls=WALLS, **KW)
    assert float(np.max(np.abs(w[1] - plain[1]))) > 1e-3              # the ports are active in the run the strips are held to
    with lbm.Group(NX, NY, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(STEPS, OF)
        assert g.first_unstable_step() == -1
        assert [c.ports() for c in g.ctxs] == [((PRESSURE, 1.015), (VELOCITY, 0.03))] * nstrips
        assert_group_is_whole(g, w)


# ---- 6. the snapshot and its consumers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "fast-rowil-col6"])
def test_macros_on_the_port_columns(lbm, plan, name):
    """After step(n, of), macros() on both port columns is (rho, u, 0) of the rule: the given one exactly, the solved one at the bars."""
    ref, _ = pair_reference(name)
    _, (rho, ux, uy), _, _ = run_plan(lbm, NX, NY, plan, STEPS, OF, ports=PAIRS[name], walls=WALLS, **KW)
    west, east = PAIRS[name]
    rho_bar = 1e-14 if strict(plan) else 1e-10
    for x, port in ((0, west), (NX - 1, east)):
        kind = VELOCITY if port == VELOCITY else port[0]
        assert np.all(uy[:, x] == 0.0)
        if kind == PRESSURE:
            assert np.array_equal(rho[:, x], ref.rho[:, x]) and np.all(rho[:, x] == port[1])
            assert float(np.max(np.abs(ux[:, x] - ref.ux[:, x]))) <= U_BAR_ABS
        else:
            assert np.array_equal(ux[:, x], ref.ux[:, x]) and np.all(ux[:, x] == (KW["inlet_velocity"] if x == 0 else port[1]))
            assert float(np.max(np.abs(rho[:, x] - ref.rho[:, x]))) <= rho_bar


REPORT_KW = dict(walls=WALLS, ports=((PRESSURE, 1.015), (VELOCITY, 0.03)), **KW)
REPORT_NX, REPORT_NY = 128, 48


@functools.lru_cache(maxsize=None)
def twin_macros(lbm, steps):
    with lbm.Context(REPORT_NX, REPORT_NY, **REPORT_KW) as twin:
        twin.initialise()
        twin.step(steps, 0)
        return twin.macros()


def test_statistics_frame_and_probes_equal_macros_one_step_later(lbm):
    nx, ny = REPORT_NX, REPORT_NY
    pts = [(0, y) for y in (0, 7, ny // 2, ny - 1)] + [(nx - 1, y) for y in (0, 11, ny // 2, ny - 1)]
    with lbm.Context(nx, ny, frames=1, probes=np.array(pts, dtype=np.float64), **REPORT_KW) as ctx:
        ctx.initialise()
        ctx.stats_begin(40)
        ctx.step(41, 40)                   # one statistics sample, at t = 40; frames and probes at t = 0 and 40
        assert ctx.stats_samples() == 1
        sums = ctx.stats_sums()
        frames = ctx.drain_frames()
        ts, vals = ctx.drain_probes()
    rho, ux, uy = twin_macros(lbm, 41)
    assert np.all(rho[:, 0] == 1.015) and np.all(ux[:, -1] == 0.03)
    for got, want in zip(sums, (rho, ux, uy, ux * ux, uy * uy, ux * uy)):
        assert np.array_equal(got, want)
    assert [t for t, _ in frames] == [0, 40] and list(ts) == [0, 40]
    for got, want in zip(frames[1][1][:3], (rho, ux, uy)):
        assert np.array_equal(got, want.astype(np.float32))
    for j, (x, y) in enumerate(pts):
        assert np.array_equal(vals[1, j], np.array([rho[y, x], ux[y, x], uy[y, x]])), (x, y)


# ---- 7. checkpoints -----------------------------------------------------------------------------------------------------------------------
def test_ports_checkpoint_round_trip_handover_and_refusals(lbm, tmp_path):
    nx, ny = NX, NY
    ports = ((PRESSURE, 1.01), (PRESSURE, 0.99))
    sched = np.linspace(0.5, 1.0, 9)
    path = tmp_path / "ports.ckpt"
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], ports=ports, walls=WALLS, **KW) as a:
        a.initialise()
        a.step(37, 0)
        a.save_state(path)
        a.step(30, 10)
        assert a.first_unstable_step() == -1
        ref = (a.populations("f_next"), a.drain_force_log())
        a.load_state(path)                                                       # resumed in place
        a.step(30, 10)
        assert np.array_equal(a.populations("f_next"), ref[0]) and a.drain_force_log() == ref[1]
    data = open(path, "rb").read()
    # magic, fixed header (72 bytes), flags (walls 16 | ports 256), the walls' four doubles, the ports' four doubles
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q4d4d", data[72:144]) == (16 | 256, 1.0, 0.0, 2.0, 0.05, 1.0, 1.01, 1.0, 0.99)
    assert len(data) == 144 + 9 * nx * ny * 8
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], ports=ports, walls=WALLS, **KW) as b:      # handed to another family
        b.initialise()
        b.load_state(path)
        b.step(30, 10)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, walls=WALLS, **KW) as c:                                                      # default ports
        c.initialise()
        with pytest.raises(lbm.LbmError, match="with ports west kind 1 value 1.01, east kind 1 value 0.99; this context has the default ports"):
            c.load_state(path)
        c.step(3, 0)
        c.save_state(tmp_path / "plain.ckpt")
    with lbm.Context(nx, ny, ports=((PRESSURE, 1.01), (VELOCITY, 0.03)), walls=WALLS, **KW) as d:         # other ports
        d.initialise()
        with pytest.raises(lbm.LbmError, match="with ports west kind 1 value 1.01, east kind 1 value 0.99; this context has ports west kind 1 "
                                               "value 1.01, east kind 0 value 0.03"):
            d.load_state(path)
        with pytest.raises(lbm.LbmError, match="with the default ports; this context has ports west kind 1 value 1.01, east kind 0 value 0.03"):
            d.load_state(tmp_path / "plain.ckpt")
    # behind a schedule's digest (a west velocity port takes one)
    with lbm.Context(nx, ny, ports=(VELOCITY, (VELOCITY, 0.04)), inlet_schedule=sched, **KW) as e:
        e.initialise()
        e.step(5, 0)
        e.save_state(tmp_path / "sched.ckpt")
    head = open(tmp_path / "sched.ckpt", "rb").read(128)
    assert struct.unpack("<Q", head[72:80]) == (32 | 256,) and struct.unpack("<4d", head[88:120]) == (0.0, 0.0, 0.0, 0.04)


# ---- 8. the defaults are today's code ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["rowil-site-nt", "planar-pair8-nt", "planar-fuse3-8", "rowil-fuse4-nt-xcd", "rowil-deep6-nt", "rowil-col5-nt",
                                  "fast-rowil-col6", "park10"])
def test_default_ports_are_no_ports(lbm, plan, tmp_path):
    out = []
    for k, extra in enumerate(({}, dict(ports=None), dict(ports=(VELOCITY, (PRESSURE, 1.0))), dict(ports=(None, None)))):
        with lbm.Context(NX, NY, options=fc.plan_options(plan), walls=WALLS, **KW, **extra) as ctx:
            if k == 3:                                                           # set, then set back
                ctx.set_port("west", PRESSURE, 1.02)
                ctx.set_port("east", VELOCITY, 0.01)
                ctx.set_port("west", VELOCITY)
                ctx.set_port("east", PRESSURE, 1.0)
            assert ctx.ports() == ((VELOCITY, 0.0), (PRESSURE, 1.0))
            ctx.initialise()
            ctx.step(STEPS, OF)
            ctx.save_state(tmp_path / ("d%d.ckpt" % k))
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.populations("f_current"),
                        open(tmp_path / ("d%d.ckpt" % k), "rb").read()))
    a = out[0]
    ref = oracle_run(NX, NY, STEPS, OF, walls=WALLS, **KW)
    assert_matches_reference(fc.contracted(plan), a[1], a[2], a[3], ref, U_BAR_ABS)
    for b in out[1:]:
        assert a[0] == b[0] and a[3] == b[3] and a[5] == b[5]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y)
    with lbm.Context(NX, NY, options=fc.plan_options(plan), **KW) as ctx:       # without walls: an LBMCKPT1 head
        ctx.set_port("east", PRESSURE, 1.0)
        ctx.initialise()
        ctx.step(2, 0)
        ctx.save_state(tmp_path / "v1.ckpt")
    assert open(tmp_path / "v1.ckpt", "rb").read(8) == b"LBMCKPT1"


# ---- 9. the pressure-driven channel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["rowil-deep6-nt", "fast-rowil-deep7"])
def test_pressure_driven_channel(lbm, plan):
    nx, ny, tau = CHANNEL["nx"], CHANNEL["ny"], CHANNEL["tau"]
    ref = channel_run(6000)
    assert ref.first_unstable == -1
    fn, macros, log, _ = run_plan(lbm, nx, ny, plan, 6000, 0, ports=CHANNEL["ports"], solid=np.zeros((ny, nx), np.uint8), tau=tau, inlet_velocity=0.0)
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)
    mid = macros[1][:, nx // 2]
    G, H, nu = (1.005 - 0.995) / (3.0 * (nx - 1)), ny - 1, (tau - 0.5) / 3.0
    ratio = float(mid[ny // 2]) / (G * H * H / (8.0 * nu))
    print("channel on %s: centreline ratio %.4f" % (plan, ratio))
    assert np.all(mid[1:-1] > 0.0) and 0.85 < ratio < 1.0


# ---- 10. arguments ------------------------------------------------------------------------------------------------------------------------
def test_set_port_arguments(lbm):
    with lbm.Context(128, 32) as ctx:
        L = ctx.L
        k, v = C.c_int(-7), C.c_double(-7.0)
        assert ctx.ports() == ((VELOCITY, 0.0), (PRESSURE, 1.0))
        for side in (-1, 2):
            assert L.lbm_set_port(ctx.h, side, 1, 1.0) == -1 and b"side" in L.lbm_last_error()
            assert L.lbm_get_port(ctx.h, side, C.byref(k), C.byref(v)) == -1 and b"side" in L.lbm_last_error()
        for kind in (-1, 2):
            assert L.lbm_set_port(ctx.h, 0, kind, 1.0) == -1 and b"kind" in L.lbm_last_error()
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert L.lbm_set_port(ctx.h, 1, 1, bad) == -1 and b"value" in L.lbm_last_error()
        for bad in (0.0, -1.0):
            assert L.lbm_set_port(ctx.h, 0, 1, bad) == -1 and b"pressure" in L.lbm_last_error()
        for bad in (1.0, -1.0, 3.0):
            assert L.lbm_set_port(ctx.h, 1, 0, bad) == -1 and b"east velocity" in L.lbm_last_error()
        assert L.lbm_set_port(ctx.h, 0, 0, 0.01) == -1 and b"west velocity port" in L.lbm_last_error()
        assert ctx.ports() == ((VELOCITY, 0.0), (PRESSURE, 1.0))            # a refused call changes nothing
        ctx.set_port("east", VELOCITY, -0.25)
        assert L.lbm_get_port(ctx.h, 1, None, None) == 0                     # both pointers are nullable
        assert L.lbm_get_port(ctx.h, 1, C.byref(k), None) == 0 and k.value == 0
        assert L.lbm_get_port(ctx.h, 1, None, C.byref(v)) == 0 and v.value == -0.25
        ctx.set_port("east", PRESSURE, 0.99)
        ctx.initialise()
        assert L.lbm_set_port(ctx.h, 0, 1, 1.0) == -1 and b"before lbm_initialise" in L.lbm_last_error()
        assert ctx.ports() == ((VELOCITY, 0.0), (PRESSURE, 0.99))


def test_a_west_pressure_port_takes_no_inlet_velocity(lbm):
    with lbm.Context(64, 32, ports=((PRESSURE, 1.01), None), inlet_profile=lbm.parabolic_profile(32, 0.02), inlet_velocity=0.02) as ctx:
        with pytest.raises(lbm.LbmError, match="inlet profile.*west pressure port"):
            ctx.initialise()
    with lbm.Context(64, 32, ports=((PRESSURE, 1.01), None), inlet_schedule=[0.5, 1.0]) as ctx:
        with pytest.raises(lbm.LbmError, match="inlet schedule.*west pressure port"):
            ctx.initialise()
    with lbm.Context(64, 32, ports=(VELOCITY, (VELOCITY, 0.02)), inlet_schedule=[0.5, 1.0]) as ctx:       # a velocity inlet takes both
        ctx.initialise()


# ---- 11. lbm_solver -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strips", [1, 2])
def test_lbm_solver_runs_the_ports_and_writes_them(lbm, tmp_path, strips):
    nx, ny, steps, tau = 64, 33, 41, 0.8
    args = ["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", "20", "--tau", str(tau), "--inlet-velocity", "0",
            "--cylinder-radius", "0", "--no-vtk", "--no-tune", "--inlet", "pressure:1.005", "--outlet", "pressure:0.995"]
    pr = run_solver(args + (["--strips", "2"] if strips == 2 else []), tmp_path)
    assert "Ports: inlet pressure:1.005, outlet pressure:0.995" in pr.stdout
    params = read_params(tmp_path / "simulation_params.csv")
    assert (params["inlet"], params["outlet"]) == ("pressure:1.005", "pressure:0.995")
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=0.0, cylinder_radius=0.0, ports=((PRESSURE, 1.005), (PRESSURE, 0.995)), options=dict(tune=0)) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        rho, ux, uy = ctx.macros()
    cux, cuy, crho = read_velocity_field(tmp_path / "velocity_field.csv", nx, ny)
    for got, want in ((cux, ux), (cuy, uy), (crho, rho)):
        assert np.max(np.abs(got - want)) <= 5.1e-9
    assert np.all(np.abs(crho[:, 0] - 1.005) <= 5.1e-9) and np.all(np.abs(crho[:, -1] - 0.995) <= 5.1e-9)


def test_lbm_solver_with_default_ports_says_nothing_about_ports(lbm, tmp_path):
    pr = run_solver(["--nx", "64", "--ny", "32", "--steps", "11", "--output-frequency", "5", "--no-vtk", "--inlet", "velocity", "--outlet", "pressure:1"], tmp_path)
    assert "Ports:" not in pr.stdout
    assert not any(k in ("inlet", "outlet") for k in read_params(tmp_path / "simulation_params.csv"))
