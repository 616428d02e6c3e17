"""The uniform driving force (lbm_set_forcing, Context/Group(forcing=...), lbm_solver --forcing) on the GPU.

The reference operator is guo_collide of tests/forcing_reference.py: numpy, fp64, IEEE, in the operation order the library's strict
arithmetic evaluates (lbm_kernels.hpp bgk_collide, the ar_forced phase). It replaces o.collide() in the stepwise oracle loop
(tests/reference.py oracle_run), as trt_collide does for TRT; oracle/ is untouched. Strict plans must match it bit for bit, contracted
ones within 1e-10. tests/test_forcing_cpu.py holds the operator itself to its conservation laws and to a channel flow."""
import functools
import importlib
import struct

import numpy as np
import pytest

from tests.forcing_reference import guo_collide
from tests.helpers import (ORACLE_PLANS, PKG, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, host_staged_two_strips,  # noqa: F401
                           lbm_gpu, read_csv_rows, read_params, read_velocity_field, record, run_solver, solver, square, whole_run)
from tests.reference import CX, CY, oracle_run

pytestmark = pytest.mark.gpu

F = (2e-5, -1e-5)


# ---- 1. every plan against the reference ----------------------------------------------------------------------------------------
NX, NY, STEPS, OF = 160, 48, 240, 60
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
CASES = ["disc", "square", "disc-parabolic"]
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))


def case_inputs(name, lbm):
    mask = square(NX, NY) if name == "square" else None
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"]) if name == "disc-parabolic" else None
    return mask, u


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the forced reference run, max |f_forced - f_bgk| against the oracle's own BGK on the same case); computed on the CPU, once."""
    lbm = importlib.import_module(PKG)
    mask, u = case_inputs(name, lbm)
    ref = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, collide=functools.partial(guo_collide, force=F), **KW)
    bgk = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, **KW)
    return ref, float(np.max(np.abs(ref.f_next - bgk.f_next)))


@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("name", CASES)
def test_forcing_against_the_reference(lbm, name, plan):
    mask, u = case_inputs(name, lbm)
    for other in CASES:                               # precondition, on the CPU before any GPU run: stable, and not BGK
        ref_o, away = reference(other)
        assert ref_o.first_unstable == -1, other
        assert away > 1e-6, (other, away)             # the force is felt: the test cannot pass with it doing nothing
    ref, _ = reference(name)
    with lbm.Context(NX, NY, options=PLANS[plan], solid=mask, inlet_profile=u, forcing=F, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        assert ctx.forcing() == F
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
        assert ctx.kernel_name().endswith((",8>", ",9>")), ctx.kernel_name()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 2. the tall shapes ---------------------------------------------------------------------------------------------------------------
# collision_models (csrc/lbm_plan.hpp): the forced row grants the tall fp64 regions (deep 10 / 11) and, like LES and TRT, not the tall
# fp32 ones (deep 8). The grids are the smallest of tests/test_gpu_col_parked.py: partial last bands and columns at both depths.
PIN = dict(tune=0, layout=1, pair_ty=12, xcd=1, arith=1)


@functools.lru_cache(maxsize=None)
def col6_run(lbm, nx, ny):
    """The forced fast-rowil-col6 plan at 20 + 13 iterations: what the tall shapes must equal."""
    with lbm.Context(nx, ny, options=PLANS["fast-rowil-col6"], inlet_velocity=0.05, forcing=F) as ctx:
        ctx.initialise()
        ctx.step(20, 0)
        ctx.step(13, 5)
        assert ctx.kernel_name().endswith(",9>")
        return ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()


@pytest.mark.parametrize("deep", [10, 11])
@pytest.mark.parametrize("grid", [(118, 64), (130, 69), (130, 70)], ids=lambda g: "%dx%d" % g)
def test_tall_fp64_regions_equal_the_col6_plan(lbm, grid, deep):
    nx, ny = grid
    want = col6_run(lbm, nx, ny)
    with lbm.Context(nx, ny, options=dict(PIN, nt=0, ntl=1, alternate=1, deep=deep), inlet_velocity=0.05, forcing=F) as ctx:
        ctx.initialise()
        ctx.step(20, 0)
        ctx.step(13, 5)
        assert ctx.first_unstable_step() == -1
        assert ctx.kernel_name().startswith("k_stepc_col<double,5,8,") and ctx.kernel_name().endswith(",9>"), ctx.kernel_name()
        assert np.array_equal(ctx.populations("f_next"), want[0])
        for a, b in zip(ctx.macros(), want[1]):
            assert np.array_equal(a, b)
        assert ctx.drain_force_log() == want[2]


def test_fp32_forcing_has_no_tall_regions(lbm):
    with lbm.Context(256, 64, precision="f32", forcing=F) as ctx:
        with pytest.raises(lbm.LbmError, match=r"deep 8 \(64x48 regions in registers\) has no forced BGK"):
            ctx.set_option("deep", 8)
    with lbm.Context(256, 64, precision="f32", options=dict(tune=0, deep=8)) as ctx:
        with pytest.raises(lbm.LbmError, match=r"deep 8 \(64x48 regions in registers\) has no forced BGK"):
            ctx.set_forcing(*F)
        ctx.set_option("deep", 0)
        ctx.set_forcing(*F)


# ---- 3. forcing = (0, 0) is BGK ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col5-nt", "planar-fuse3-8", "fast-rowil-col6", "rowil-deep6-nt", "planar-site"])
def test_zero_forcing_is_bgk(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in ({}, dict(forcing=(0.0, 0.0))):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            assert ctx.forcing() == (0.0, 0.0)
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()))
    a, b = out
    assert a[0] == b[0] and a[0].endswith((",0>", ",1>"))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    with lbm.Context(nx, ny, options=PLANS[plan], forcing=F, **kw) as ctx:     # set, then cleared
        ctx.set_forcing(0.0, 0.0)
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.kernel_name() == a[0] and np.array_equal(ctx.populations("f_next"), a[1])
        for x, y in zip(ctx.macros(), a[2]):
            assert np.array_equal(x, y)
        assert ctx.drain_force_log() == a[3]


# ---- 4. invariance within a mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_forced_context(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1, forcing=F)
    w = whole_run(lbm, nx, ny, plan, steps, of, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert all(c.forcing() == F and c.kernel_name().endswith((",8>", ",9>")) for c in g.ctxs)
        assert_group_is_whole(g, w)


def test_host_staged_forced_strips(lbm):
    nx, ny = 512, 256
    kw = dict(tau=0.55, inlet_velocity=0.08, forcing=F)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, None, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 5. the snapshot ------------------------------------------------------------------------------------------------------------------
SNAP = dict(tau=0.55, inlet_velocity=0.06, forcing=F)
SNX, SNY, ST = 128, 48, 40


@functools.lru_cache(maxsize=None)
def snapshot_twin(lbm):
    """macros() of a forced context with steps_done == ST + 1: what every sample of iteration ST must equal."""
    with lbm.Context(SNX, SNY, **SNAP) as twin:
        twin.initialise()
        twin.step(ST + 1, 0)
        return twin.macros()


def test_statistics_frame_and_probe_equal_macros_one_step_later(lbm):
    rho, ux, uy = snapshot_twin(lbm)
    xs, ys = np.meshgrid(np.arange(0, SNX, 9), np.arange(0, SNY, 5))
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)          # on-node probes: no interpolation
    with lbm.Context(SNX, SNY, **SNAP) as ctx:
        ctx.initialise()
        ctx.stats_begin(ST)
        ctx.frames_begin(1)
        ctx.probes_begin(xy)
        ctx.step(ST + 1, ST)                   # one sample of each, at t = ST (iteration 0 lies before stats_begin's first step)
        assert ctx.kernel_name().endswith((",8>", ",9>"))
        assert ctx.stats_samples() == 1
        sums = ctx.stats_sums()
        frames = [fr for fr in ctx.drain_frames() if fr[0] == ST]
        ts, vals = ctx.drain_probes()
    for got, want in zip(sums, (rho, ux, uy, ux * ux, uy * uy, ux * uy)):
        assert np.array_equal(got, want)
    assert len(frames) == 1
    for j, want in enumerate((rho, ux, uy)):
        assert np.array_equal(frames[0][1][j], want.astype(np.float32)), j
    k = ts.tolist().index(ST)
    ix, iy = xy[:, 0].astype(int), xy[:, 1].astype(int)
    for j, want in enumerate((rho, ux, uy)):
        assert np.array_equal(vals[k][:, j], want[iy, ix]), j


@pytest.mark.parametrize("plan", ["rowil-site-nt", "fast-rowil-col6"])
def test_macros_take_half_the_force_off_the_post_collision_momentum(lbm, plan):
    """macros() and populations("f_next") read the same buffer, the post-collision populations of the last collision: their momentum
    is the pre-collision one plus F, Guo's velocity (pre + F/2) / rho = (post - F/2) / rho. With the sign flipped the two would differ by
    3/2 F."""
    with lbm.Context(SNX, SNY, options=PLANS[plan], **SNAP) as ctx:
        ctx.initialise()
        ctx.step(ST + 1, 0)
        rho, ux, uy = ctx.macros()
        fn = ctx.populations("f_next")[1:-1, 1:-1]
        solid = ctx.solid().astype(bool)
    inner = ~solid
    inner[:, 0] = inner[:, -1] = False          # the inlet and outlet columns report their boundary values
    r = sum(fn[..., i] for i in range(9))
    jx = sum(float(CX[i]) * fn[..., i] for i in range(9))
    jy = sum(float(CY[i]) * fn[..., i] for i in range(9))
    assert np.max(np.abs(rho - r)[inner]) <= 1e-14
    for u, j, f in ((ux, jx, F[0]), (uy, jy, F[1])):
        d = (j - u * rho)[inner]                # F/2 to rounding: sums of nine populations below 0.5 and one division, a few 1e-16
        assert np.max(np.abs(d - 0.5 * f)) <= 1e-15, (float(np.min(d)), float(np.max(d)), 0.5 * f)


# ---- 6. fp32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_forcing_against_fp64(lbm, arith):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05, forcing=F)     # tau: the default, 0.6, as in test_gpu_parity.py's fp32 comparison
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=dict(arith=arith), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        assert ctx.kernel_name().endswith("%d>" % (8 + arith))
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("forcing_fp32_vs_fp64_arith%d" % arith, err_rho=er, err_u=eu)
    assert er < 2e-5 and eu < 2e-4, (er, eu)     # the fp32 bars of tests/test_gpu_parity.py


# ---- 7. checkpoints -----------------------------------------------------------------------------------------------------------------
def test_forcing_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(tau=0.55, inlet_velocity=0.07)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], forcing=F, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "forced.ckpt")
        a.step(100, 50)
        assert a.first_unstable_step() == -1
        ref = (a.populations("f_next"), a.drain_force_log())
    data = open(tmp_path / "forced.ckpt", "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word, then (nothing the lower bits announce) the force
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (64,) + F
    assert len(data) == 96 + 9 * nx * ny * 8
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], forcing=F, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "forced.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:                                     # no forcing
        c.initialise()
        with pytest.raises(lbm.LbmError, match="forcing"):
            c.load_state(tmp_path / "forced.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "bgk.ckpt")
    assert open(tmp_path / "bgk.ckpt", "rb").read(8) == b"LBMCKPT1"
    with lbm.Context(nx, ny, forcing=(2e-5, 1e-5), **kw) as d:              # another force
        d.initialise()
        with pytest.raises(lbm.LbmError, match="forcing"):
            d.load_state(tmp_path / "forced.ckpt")
        with pytest.raises(lbm.LbmError, match="forcing"):
            d.load_state(tmp_path / "bgk.ckpt")
    for other in (dict(smagorinsky=0.17), dict(trt_magic=0.25)):
        with lbm.Context(nx, ny, **other, **kw) as s:
            s.initialise()
            with pytest.raises(lbm.LbmError, match="forcing"):
                s.load_state(tmp_path / "forced.ckpt")
    u = lbm.parabolic_profile(ny, 0.07)
    with lbm.Context(nx, ny, solid=square(nx, ny), inlet_profile=u, walls="free-slip", inlet_schedule=np.linspace(0.5, 1.0, 8), forcing=F, **kw) as e:
        e.initialise()                          # everything the lower bits carry, and the force behind it
        e.step(11, 0)
        e.save_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        want = e.populations("f_next")
        e.load_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        assert np.array_equal(e.populations("f_next"), want)
        with pytest.raises(lbm.LbmError):
            e.load_state(tmp_path / "forced.ckpt")
    data = open(tmp_path / "all.ckpt", "rb").read()
    flags = struct.unpack("<Q", data[72:80])[0]
    assert flags == 1 | 2 | 16 | 32 | 64
    at = 80 + 8 + 8 + 32 + 8                    # mask digest, profile digest, four doubles of the walls, schedule digest
    assert struct.unpack("<dd", data[at:at + 16]) == F and len(data) == at + 16 + 9 * nx * ny * 8


# ---- 8. arguments -------------------------------------------------------------------------------------------------------------------
def test_set_forcing_arguments(lbm):
    import ctypes as C
    with lbm.Context(128, 32) as ctx:
        L = ctx.L
        fx, fy = C.c_double(7.0), C.c_double(7.0)
        assert L.lbm_set_forcing(None, 1e-5, 0.0) == -1 and b"null" in L.lbm_last_error()
        assert L.lbm_get_forcing(None, C.byref(fx), C.byref(fy)) == -1 and b"null" in L.lbm_last_error()
        for bad in (float("nan"), float("inf"), -float("inf"), 1.0, -1.0, 2.5):
            assert L.lbm_set_forcing(ctx.h, bad, 0.0) == -1, bad
            assert b"fx" in L.lbm_last_error()
            assert L.lbm_set_forcing(ctx.h, 0.0, bad) == -1, bad
            assert b"fy" in L.lbm_last_error()
        assert ctx.forcing() == (0.0, 0.0)
        for good in ((0.0, 0.0), (2e-5, -1e-5), (-0.999, 0.999), (0.0, 1e-300)):
            assert L.lbm_set_forcing(ctx.h, *good) == 0
            assert ctx.forcing() == good
        assert L.lbm_get_forcing(ctx.h, None, None) == 0 and L.lbm_get_forcing(ctx.h, C.byref(fx), None) == 0 and fx.value == 0.0
        assert L.lbm_get_forcing(ctx.h, None, C.byref(fy)) == 0 and fy.value == 1e-300
        ctx.initialise()
        assert L.lbm_set_forcing(ctx.h, 1e-5, 0.0) == -1 and b"before lbm_initialise" in L.lbm_last_error()
        assert ctx.kernel_name().endswith(",8>")            # (0, 1e-300) is a force
    for other, setter, value in ((dict(smagorinsky=0.17), "lbm_set_smagorinsky", 0.17), (dict(trt_magic=0.25), "lbm_set_trt", 0.25)):
        with lbm.Context(128, 32, **other) as ctx:                       # LES / TRT, then a force
            assert ctx.L.lbm_set_forcing(ctx.h, *F) == -1
            assert b"cannot be combined" in ctx.L.lbm_last_error() and b"lbm_set_forcing" in ctx.L.lbm_last_error()
            assert ctx.L.lbm_set_forcing(ctx.h, 0.0, 0.0) == 0
        with lbm.Context(128, 32, forcing=F) as ctx:                     # a force, then LES / TRT
            assert getattr(ctx.L, setter)(ctx.h, value) == -1
            assert b"cannot be combined" in ctx.L.lbm_last_error() and b"forcing" in ctx.L.lbm_last_error()
            assert getattr(ctx.L, setter)(ctx.h, 0.0) == 0
        with pytest.raises(lbm.LbmError):
            lbm.Context(128, 32, forcing=F, **other)
    with pytest.raises(lbm.LbmError):
        lbm.Context(128, 32, forcing=(1.5, 0.0))


# ---- 9. the host CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
def test_lbm_solver_forcing_matches_the_binding(lbm, solver, tmp_path, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    tau, u0 = 0.55, 0.08
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--tau", str(tau),
                     "--inlet-velocity", str(u0), "--cylinder-radius", "0.1", "--no-vtk", "--forcing", "2e-5,-1e-5"] + extra, tmp_path)
    assert "driving force (Guo): Fx = 2e-05, Fy = -1e-05" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=u0, cylinder_radius=0.1, forcing=F) as ctx:
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
    assert float(params["forcing_x"]) == F[0] and float(params["forcing_y"]) == F[1]
    assert abs(float(params["tau"]) - tau) < 1e-12
