"""Smagorinsky LES collision (lbm_set_smagorinsky, Context/Group(smagorinsky=...), lbm_solver --smagorinsky) on the GPU.

The reference operator is les_collide of tests/reference.py: numpy, fp64, IEEE, in the operation order the library's strict arithmetic
evaluates (lbm_kernels.hpp les_tau_inv_strict). It replaces o.collide() in the stepwise oracle loop (oracle_run there); oracle/ is
untouched. Strict plans must match it bit for bit, contracted ones within 1e-10."""
import functools
import importlib

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PKG, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, host_staged_two_strips,  # noqa: F401
                           lbm_gpu, read_csv_rows, read_params, read_velocity_field, record, run_solver, square, whole_run)
from tests.reference import les_collide, oracle_run

pytestmark = pytest.mark.gpu


# ---- 1 / 2. every plan against the reference ----------------------------------------------------------------------------------
NX, NY, STEPS, OF, CS = 160, 48, 240, 60, 0.17
KW = dict(tau=0.51, inlet_velocity=0.08, cylinder_radius=0.1)
CASES = ["disc", "square", "disc-parabolic"]
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))


def case_inputs(name, lbm):
    mask = square(NX, NY) if name == "square" else None
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"]) if name == "disc-parabolic" else None
    return mask, u


@functools.lru_cache(maxsize=None)
def reference(name):
    lbm = importlib.import_module(PKG)
    mask, u = case_inputs(name, lbm)
    return oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, collide=functools.partial(les_collide, cs=CS), **KW)


@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("name", CASES)
def test_les_against_the_reference(lbm, name, plan):
    mask, u = case_inputs(name, lbm)
    ref = reference(name)
    assert ref.first_unstable == -1
    assert ref.tau_max - KW["tau"] > 1e-3, ref.tau_max          # the model is active: the test cannot pass with LES doing nothing
    with lbm.Context(NX, NY, options=PLANS[plan], solid=mask, inlet_profile=u, smagorinsky=CS, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
        assert ctx.kernel_name().endswith((",2>", ",3>")), ctx.kernel_name()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_les_against_fp64(lbm, arith):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05, smagorinsky=CS)       # (the flow of test_gpu_inlet_profile.py's fp32 test, with the model on)
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=dict(arith=arith), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        assert ctx.kernel_name().endswith("%d>" % (2 + arith))
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("les_fp32_vs_fp64_arith%d" % arith, err_rho=er, err_u=eu)
    assert er < 2e-5 and eu < 2e-4, (er, eu)     # the fp32 bars of tests/test_gpu_parity.py


def test_fp32_les_has_no_tall_regions(lbm):
    with lbm.Context(256, 64, precision="f32", smagorinsky=CS) as ctx:
        with pytest.raises(lbm.LbmError, match="no Smagorinsky"):
            ctx.set_option("deep", 8)
    with lbm.Context(256, 64, precision="f32", options=dict(tune=0, deep=8)) as ctx:
        ctx.set_smagorinsky(CS)
        with pytest.raises(lbm.LbmError, match="no Smagorinsky"):
            ctx.initialise()


# ---- 3. invariance within a mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_les_context(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(tau=0.51, inlet_velocity=0.08, cylinder_radius=0.1, smagorinsky=CS)
    w = whole_run(lbm, nx, ny, plan, steps, of, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)


@pytest.mark.parametrize("plan", [None, "rowil-col5-nt", "fast-rowil-col6"])
def test_host_staged_les_strips(lbm, plan):
    nx, ny = 512, 256
    kw = dict(tau=0.51, inlet_velocity=0.08, smagorinsky=CS)
    ref_plan = "fast-site" if plan and plan.startswith("fast") else "rowil-site-nt"
    with lbm.Context(nx, ny, options=PLANS[ref_plan], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, PLANS[plan] if plan else None, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 4. Cs = 0 is BGK ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col5-nt", "planar-fuse3-8", "fast-rowil-col6", "rowil-deep6-nt", "planar-site"])
def test_cs_zero_is_bgk(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in ({}, dict(smagorinsky=0.0)):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()))
    a, b = out
    assert a[0] == b[0] and not a[0].endswith((",2>", ",3>"))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    with lbm.Context(nx, ny, options=PLANS[plan], smagorinsky=CS, **kw) as ctx:     # Cs set, then cleared
        ctx.set_smagorinsky(0.0)
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.kernel_name() == a[0] and np.array_equal(ctx.populations("f_next"), a[1])


# ---- 5. stabilisation ----------------------------------------------------------------------------------------------------------
STAB = dict(tau=0.505, inlet_velocity=0.1)


def first_unstable(lbm, cs, arith=0, steps=4000):
    extra = dict(smagorinsky=cs) if cs else {}
    with lbm.Context(400, 100, options=dict(arith=arith), **STAB, **extra) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        return ctx.first_unstable_step()


def test_bgk_diverges_where_the_oracle_does(lbm):
    want = oracle_run(400, 100, 4000, 0, **STAB).first_unstable
    assert 0 <= want < 4000
    assert first_unstable(lbm, 0.0) == want


@pytest.mark.parametrize("arith", [0, 1])
def test_les_017_is_stable(lbm, arith):
    assert first_unstable(lbm, 0.17, arith) == -1


def test_les_010_diverges_where_the_reference_does(lbm):
    want = oracle_run(400, 100, 4000, 0, collide=functools.partial(les_collide, cs=0.10), **STAB).first_unstable
    assert 0 <= want < 4000
    record("les_stabilisation", first_unstable_les_010=want)
    assert first_unstable(lbm, 0.10) == want


# ---- 6. checkpoints ------------------------------------------------------------------------------------------------------------
def test_les_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(tau=0.52, inlet_velocity=0.07)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], smagorinsky=CS, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "les.ckpt")
        a.step(100, 50)
        ref = (a.populations("f_next"), a.drain_force_log())
    data = open(tmp_path / "les.ckpt", "rb").read()
    assert data[:8] == b"LBMCKPT3"
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], smagorinsky=CS, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "les.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="Smagorinsky constant"):
            c.load_state(tmp_path / "les.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "bgk.ckpt")
    assert open(tmp_path / "bgk.ckpt", "rb").read(8) == b"LBMCKPT1"
    with lbm.Context(nx, ny, smagorinsky=0.1, **kw) as d:
        d.initialise()
        with pytest.raises(lbm.LbmError, match="Smagorinsky constant"):
            d.load_state(tmp_path / "les.ckpt")
        with pytest.raises(lbm.LbmError, match="Smagorinsky constant"):
            d.load_state(tmp_path / "bgk.ckpt")
    u = lbm.parabolic_profile(ny, 0.07)
    mask = square(nx, ny)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, smagorinsky=CS, **kw) as e:   # all three flags
        e.initialise()
        e.step(11, 0)
        e.save_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        want = e.populations("f_next")
        e.load_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        assert np.array_equal(e.populations("f_next"), want)
        with pytest.raises(lbm.LbmError):
            e.load_state(tmp_path / "les.ckpt")


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------
def test_set_smagorinsky_arguments(lbm):
    with lbm.Context(128, 32) as ctx:
        L = ctx.L
        assert L.lbm_set_smagorinsky(None, 0.1) == -1 and b"null" in L.lbm_last_error()
        for bad in (float("nan"), float("inf"), -float("inf"), -0.1, -1e-300, 1.0000001, 2.0):
            assert L.lbm_set_smagorinsky(ctx.h, bad) == -1, bad
            assert b"Cs" in L.lbm_last_error()
        for good in (0.0, 1.0, 0.17):
            assert L.lbm_set_smagorinsky(ctx.h, good) == 0
        ctx.initialise()
        assert L.lbm_set_smagorinsky(ctx.h, 0.1) == -1 and b"before lbm_initialise" in L.lbm_last_error()
    with pytest.raises(lbm.LbmError):
        lbm.Context(128, 32, smagorinsky=-0.5)


# ---- 8. the host CLI -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
def test_lbm_solver_smagorinsky_matches_the_binding(lbm, tmp_path, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    tau, u0 = 0.51, 0.08
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--tau", str(tau),
                     "--inlet-velocity", str(u0), "--cylinder-radius", "0.1", "--no-vtk", "--smagorinsky", "0.17"] + extra, tmp_path)
    assert "Smagorinsky LES, Cs = 0.17" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=u0, cylinder_radius=0.1, smagorinsky=0.17) as ctx:
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
    assert abs(float(params["smagorinsky_cs"]) - 0.17) < 1e-12
    assert abs(float(params["tau"]) - tau) < 1e-12
