"""Two-relaxation-time collision (lbm_set_trt, Context/Group(trt_magic=...), lbm_solver --trt-magic) on the GPU.

The reference operator is trt_collide of tests/reference.py: numpy, fp64, IEEE, in the operation order the library's strict arithmetic
evaluates (lbm_kernels.hpp bgk_collide, the ar_trt branch of `pair`). It replaces o.collide() in the stepwise oracle loop (oracle_run
there), as les_collide does for the Smagorinsky operator; oracle/ is untouched. Strict plans must match it bit for bit,
contracted ones within 1e-10."""
import functools
import importlib
import struct

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PKG, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, host_staged_two_strips,  # noqa: F401
                           lbm_gpu, read_csv_rows, read_params, read_velocity_field, record, run_solver, square, whole_run)
from tests.reference import oracle_run, trt_collide

pytestmark = pytest.mark.gpu


# ---- 1. every plan against the reference ----------------------------------------------------------------------------------------
NX, NY, STEPS, OF, MAGIC = 160, 48, 240, 60, 3.0 / 16.0
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
CASES = ["disc", "square", "disc-parabolic"]
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))


def case_inputs(name, lbm):
    mask = square(NX, NY) if name == "square" else None
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"]) if name == "disc-parabolic" else None
    return mask, u


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the TRT reference run, max |f_trt - f_bgk| against the oracle's own BGK on the same case); computed on the CPU, once."""
    lbm = importlib.import_module(PKG)
    mask, u = case_inputs(name, lbm)
    ref = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, collide=functools.partial(trt_collide, magic=MAGIC), **KW)
    bgk = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, **KW)
    return ref, float(np.max(np.abs(ref.f_next - bgk.f_next)))


@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("name", CASES)
def test_trt_against_the_reference(lbm, name, plan):
    mask, u = case_inputs(name, lbm)
    for other in CASES:                               # precondition, on the CPU before any GPU run: stable, and not BGK
        ref_o, away = reference(other)
        assert ref_o.first_unstable == -1, other
        assert away > 1e-6, (other, away)             # the operator is active: the test cannot pass with TRT doing nothing
    ref, _ = reference(name)
    with lbm.Context(NX, NY, options=PLANS[plan], solid=mask, inlet_profile=u, trt_magic=MAGIC, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
        assert ctx.kernel_name().endswith((",4>", ",5>")), ctx.kernel_name()
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 2. degenerate magic parameter: the two rates coincide, BGK up to rounding ----------------------------------------------------
def test_degenerate_magic_is_bgk_up_to_rounding(lbm):
    nx, ny, steps = 200, 64, 97
    kw = dict(tau=0.55, inlet_velocity=0.06)
    magic = (kw["tau"] - 0.5) ** 2
    # first on the CPU: trt_collide against the unmodified oracle
    two = oracle_run(nx, ny, steps, 0, collide=functools.partial(trt_collide, magic=magic), **kw).f_next
    bgk = oracle_run(nx, ny, steps, 0, **kw).f_next
    scale = float(np.max(np.abs(bgk)))
    cpu = float(np.max(np.abs(two - bgk))) / scale
    record("trt_degenerate_magic", cpu_rel=cpu)
    assert cpu <= 1e-10, cpu
    out = []
    for extra in (dict(trt_magic=magic), {}):
        with lbm.Context(nx, ny, options=dict(arith=0), **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, 0)
            out.append((ctx.kernel_name(), ctx.populations("f_next")))
    assert out[0][0].endswith(",4>") and out[1][0].endswith(",0>")
    gpu = float(np.max(np.abs(out[0][1] - out[1][1]))) / float(np.max(np.abs(out[1][1])))
    record("trt_degenerate_magic_gpu", gpu_rel=gpu)
    assert gpu <= 1e-10, gpu


# ---- 3. invariance within a mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_trt_context(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1, trt_magic=MAGIC)
    w = whole_run(lbm, nx, ny, plan, steps, of, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)


def test_host_staged_trt_strips(lbm):
    nx, ny = 512, 256
    kw = dict(tau=0.55, inlet_velocity=0.08, trt_magic=MAGIC)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, None, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 4. magic = 0 is BGK --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col5-nt", "planar-fuse3-8", "fast-rowil-col6", "rowil-deep6-nt", "planar-site"])
def test_magic_zero_is_bgk(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in ({}, dict(trt_magic=0.0)):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()))
    a, b = out
    assert a[0] == b[0] and a[0].endswith((",0>", ",1>"))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    with lbm.Context(nx, ny, options=PLANS[plan], trt_magic=MAGIC, **kw) as ctx:     # set, then cleared
        ctx.set_trt(0.0)
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.kernel_name() == a[0] and np.array_equal(ctx.populations("f_next"), a[1])
        assert ctx.drain_force_log() == a[3]


# ---- 5. stability follows the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magic", [0.25, 3.0 / 16.0])
def test_trt_stability_follows_the_reference(lbm, magic):
    stab = dict(tau=0.505, inlet_velocity=0.1)
    want = oracle_run(400, 100, 4000, 0, collide=functools.partial(trt_collide, magic=magic), **stab).first_unstable
    with lbm.Context(400, 100, options=dict(arith=0), trt_magic=magic, **stab) as ctx:
        ctx.initialise()
        ctx.step(4000, 0)
        got = ctx.first_unstable_step()
    record("trt_stability_magic_%g" % magic, reference_first_unstable=want, gpu_first_unstable=got)
    assert got == want


# ---- 6. fp32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_trt_against_fp64(lbm, arith):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05, trt_magic=0.25)     # tau: the default, 0.6, as in test_gpu_parity.py's fp32 comparison
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=dict(arith=arith), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        assert ctx.kernel_name().endswith("%d>" % (4 + arith))
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("trt_fp32_vs_fp64_arith%d" % arith, err_rho=er, err_u=eu)
    assert er < 2e-5 and eu < 2e-4, (er, eu)     # the fp32 bars of tests/test_gpu_parity.py


def test_fp32_trt_has_no_tall_regions(lbm):
    with lbm.Context(256, 64, precision="f32", trt_magic=0.25) as ctx:
        with pytest.raises(lbm.LbmError, match=r"no two-relaxation-time \(TRT\)"):
            ctx.set_option("deep", 8)
    with lbm.Context(256, 64, precision="f32", options=dict(tune=0, deep=8)) as ctx:
        with pytest.raises(lbm.LbmError, match=r"no two-relaxation-time \(TRT\)"):
            ctx.set_trt(0.25)
        ctx.set_option("deep", 0)
        ctx.set_trt(0.25)


# ---- 7. the reporting layers ride along -------------------------------------------------------------------------------------------
def test_body_rows_equal_the_force_log_under_trt(lbm):
    nx, ny = 128, 48
    labels = square(nx, ny).astype(np.int32)
    with lbm.Context(nx, ny, tau=0.55, inlet_velocity=0.06, bodies=labels, trt_magic=MAGIC) as ctx:
        ctx.initialise()
        ctx.step(121, 30)
        assert ctx.kernel_name().endswith(",4>")
        log, blog = ctx.drain_force_log(), ctx.drain_body_force_log()
    assert len(log) == 5 and [(t, fx, fy) for t, b, fx, fy in blog if b == 1] == log


def test_statistics_sample_equals_macros_one_step_later_under_trt(lbm):
    nx, ny = 128, 48
    kw = dict(tau=0.55, inlet_velocity=0.06, trt_magic=MAGIC)
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.stats_begin(40)
        ctx.step(41, 40)                   # one sample, at t = 40
        assert ctx.stats_samples() == 1
        sums = ctx.stats_sums()
    with lbm.Context(nx, ny, **kw) as twin:
        twin.initialise()
        twin.step(41, 0)
        rho, ux, uy = twin.macros()
    for got, want in zip(sums, (rho, ux, uy, ux * ux, uy * uy, ux * uy)):
        assert np.array_equal(got, want)


# ---- 8. checkpoints -----------------------------------------------------------------------------------------------------------------
def test_trt_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(tau=0.55, inlet_velocity=0.07)      # (at tau 0.52, the LES test's, this flow diverges under TRT at step 158: NaN != NaN)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], trt_magic=MAGIC, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "trt.ckpt")
        a.step(100, 50)
        assert a.first_unstable_step() == -1
        ref = (a.populations("f_next"), a.drain_force_log())
    data = open(tmp_path / "trt.ckpt", "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word, then (no digests, no Cs) the magic parameter
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qd", data[72:88]) == (8, MAGIC)
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], trt_magic=MAGIC, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "trt.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="TRT magic parameter"):
            c.load_state(tmp_path / "trt.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "bgk.ckpt")
    assert open(tmp_path / "bgk.ckpt", "rb").read(8) == b"LBMCKPT1"
    with lbm.Context(nx, ny, trt_magic=0.25, **kw) as d:
        d.initialise()
        with pytest.raises(lbm.LbmError, match="TRT magic parameter"):
            d.load_state(tmp_path / "trt.ckpt")
        with pytest.raises(lbm.LbmError, match="TRT magic parameter"):
            d.load_state(tmp_path / "bgk.ckpt")
    with lbm.Context(nx, ny, smagorinsky=0.17, **kw) as s:
        s.initialise()
        with pytest.raises(lbm.LbmError, match="TRT magic parameter"):
            s.load_state(tmp_path / "trt.ckpt")
    u = lbm.parabolic_profile(ny, 0.07)
    mask = square(nx, ny)
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, trt_magic=MAGIC, **kw) as e:   # mask + profile + TRT
        e.initialise()
        e.step(11, 0)
        e.save_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        want = e.populations("f_next")
        e.load_state(tmp_path / "all.ckpt")
        e.step(5, 0)
        assert np.array_equal(e.populations("f_next"), want)
        with pytest.raises(lbm.LbmError):
            e.load_state(tmp_path / "trt.ckpt")


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------
def test_set_trt_arguments(lbm):
    with lbm.Context(128, 32) as ctx:
        L = ctx.L
        assert L.lbm_set_trt(None, 0.25) == -1 and b"null" in L.lbm_last_error()
        for bad in (float("nan"), float("inf"), -float("inf"), -0.1, -1e-300, 1.0000001, 2.0):
            assert L.lbm_set_trt(ctx.h, bad) == -1, bad
            assert b"magic parameter" in L.lbm_last_error()
        for good in (0.0, 1.0, 0.25, 3.0 / 16.0):
            assert L.lbm_set_trt(ctx.h, good) == 0
        ctx.initialise()
        assert L.lbm_set_trt(ctx.h, 0.25) == -1 and b"before lbm_initialise" in L.lbm_last_error()
    with lbm.Context(128, 32, tau=0.5) as ctx:
        assert ctx.L.lbm_set_trt(ctx.h, 0.25) == -1 and b"tau" in ctx.L.lbm_last_error()
    with lbm.Context(128, 32, smagorinsky=0.17) as ctx:                  # LES, then TRT
        assert ctx.L.lbm_set_trt(ctx.h, 0.25) == -1 and b"cannot be combined" in ctx.L.lbm_last_error()
        assert ctx.L.lbm_set_trt(ctx.h, 0.0) == 0
    with lbm.Context(128, 32, trt_magic=0.25) as ctx:                    # TRT, then LES
        assert ctx.L.lbm_set_smagorinsky(ctx.h, 0.17) == -1 and b"cannot be combined" in ctx.L.lbm_last_error()
        assert ctx.L.lbm_set_smagorinsky(ctx.h, 0.0) == 0
    with pytest.raises(lbm.LbmError):
        lbm.Context(128, 32, smagorinsky=0.17, trt_magic=0.25)
    with pytest.raises(lbm.LbmError):
        lbm.Context(128, 32, trt_magic=-0.5)


# ---- 10. the host CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
def test_lbm_solver_trt_magic_matches_the_binding(lbm, tmp_path, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    tau, u0 = 0.55, 0.08
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--tau", str(tau),
                     "--inlet-velocity", str(u0), "--cylinder-radius", "0.1", "--no-vtk", "--trt-magic", "0.1875"] + extra, tmp_path)
    assert "TRT collision, magic = 0.1875" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=u0, cylinder_radius=0.1, trt_magic=0.1875) as ctx:
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
    assert abs(float(params["trt_magic"]) - 0.1875) < 1e-12
    assert abs(float(params["tau"]) - tau) < 1e-12
