"""The MRT collision (lbm_set_mrt, Context / Group(mrt=(bulk_rate, magic)), lbm_solver --mrt) on the GPU.

The reference operator is mrt_collide of tests/mrt_reference.py: numpy, fp64, IEEE, in the operation order the library's strict
arithmetic evaluates (lbm_kernels.hpp bgk_collide, the ar_mrt branch of `pair`). It replaces o.collide() in the stepwise reference loops
(oracle_run, ports_run, periodic_run); oracle/ is untouched. Strict plans must match it bit for bit, contracted ones within 1e-10.

The shapes the table withholds from MRT (collision_models, csrc/lbm_plan.hpp: tall = false, park = false): "deep" 8, the fp32 64x48
regions, and "deep" 10 / 11, the fp64 64x40 regions of contracted arithmetic. No plan of tests/helpers.py PLANS pins one of them, so
section 1 leaves no plan out; test_withheld_shapes_are_refused holds their refusal."""
import functools
import struct

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, host_staged_two_strips,  # noqa: F401
                           lbm_gpu, read_csv_rows, read_params, record, run_solver, whole_run)
from tests.mrt_reference import BULK, CASES, KW, MAGIC, NX, NY, OF, STEPS, case_inputs, mrt_collide, reference
from tests.periodic_reference import periodic_run
from tests.ports_reference import PRESSURE, ports_run
from tests.reference import FREESLIP, HOLD, moving, oracle_run
from tests.test_gpu_periodic import PERIODIC_PLANS

pytestmark = pytest.mark.gpu

MRT = (BULK, MAGIC)
ENDS = (",16>", ",17>")
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))
WITHHELD = {"tall": False, "park": False}            # the flags of the MRT row; see the module's text


# ---- 1. every plan against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("name", CASES)
def test_mrt_against_the_reference(lbm, name, plan):
    mask, u = case_inputs(name)
    for other in CASES:                               # precondition, on the CPU before any GPU run: stable, and not TRT
        ref_o, away = reference(other)
        assert ref_o.first_unstable == -1, other
        assert away > 1e-6, (other, away)             # the bulk rate is active: the test cannot pass with the kernels running TRT
    ref, _ = reference(name)
    with lbm.Context(NX, NY, options=PLANS[plan], solid=mask, inlet_profile=u, mrt=MRT, **KW) as ctx:
        ctx.initialise()
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
        assert ctx.kernel_name().endswith(ENDS), ctx.kernel_name()
        assert ctx.mrt() == MRT
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


def test_withheld_shapes_are_refused(lbm):
    noun = r"no multiple-relaxation-time \(MRT\) kernel"
    assert WITHHELD == {"tall": False, "park": False}
    with lbm.Context(256, 64, precision="f32", mrt=MRT) as ctx:                                # tall: the fp32 64x48 regions
        with pytest.raises(lbm.LbmError, match=noun):
            ctx.set_option("deep", 8)
    with lbm.Context(256, 64, precision="f32", options=dict(tune=0, deep=8)) as ctx:
        with pytest.raises(lbm.LbmError, match=noun):
            ctx.set_mrt(*MRT)
        ctx.set_option("deep", 0)
        ctx.set_mrt(*MRT)
    for deep in (10, 11):                                                                        # park: the fp64 64x40 regions
        with lbm.Context(256, 96, options=dict(tune=0, arith=1, deep=deep)) as ctx:
            with pytest.raises(lbm.LbmError, match=r"deep %d \(64x40 regions in registers\) has %s" % (deep, noun)):
                ctx.set_mrt(*MRT)
        with lbm.Context(256, 96, mrt=MRT) as ctx:
            with pytest.raises(lbm.LbmError, match=r"deep %d \(64x40 regions in registers\) has %s" % (deep, noun)):
                ctx.set_option("deep", deep)


# ---- 2. special cases on the device ------------------------------------------------------------------------------------------------
def test_bulk_rate_one_over_tau_is_trt_up_to_rounding(lbm):
    nx, ny, steps = 200, 64, 97
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in (dict(mrt=(1.0 / kw["tau"], MAGIC)), dict(trt_magic=MAGIC)):
        with lbm.Context(nx, ny, options=dict(arith=0), **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, 0)
            out.append((ctx.kernel_name(), ctx.populations("f_next")))
    assert out[0][0].endswith(",16>") and out[1][0].endswith(",4>")
    gpu = float(np.max(np.abs(out[0][1] - out[1][1]))) / float(np.max(np.abs(out[1][1])))
    record("mrt_bulk_rate_one_over_tau_gpu", gpu_rel=gpu)
    assert gpu <= 1e-10, gpu


# ---- 3. strips ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd", "fast-rowil-col6", "rowil-site-nt"])
def test_group_strips_are_one_mrt_context(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1, mrt=MRT)
    w = whole_run(lbm, nx, ny, plan, steps, of, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert all(c.kernel_name().endswith(ENDS) and c.mrt() == MRT for c in g.ctxs)
        assert_group_is_whole(g, w)


def test_host_staged_mrt_strips(lbm):
    nx, ny = 512, 256
    kw = dict(tau=0.55, inlet_velocity=0.08, mrt=MRT)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, None, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 4. bulk_rate = 0 is BGK ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col5-nt", "planar-fuse3-8", "fast-rowil-col6", "rowil-deep6-nt", "planar-site"])
def test_bulk_rate_zero_is_bgk(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    out = []
    for extra in ({}, dict(mrt=(0.0, MAGIC))):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw, **extra) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            assert ctx.mrt() == (0.0, 0.0)
            out.append((ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()))
    a, b = out
    assert a[0] == b[0] and a[0].endswith((",0>", ",1>"))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)
    with lbm.Context(nx, ny, options=PLANS[plan], mrt=MRT, **kw) as ctx:     # set, then cleared
        ctx.set_mrt(0.0, 0.0)
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.kernel_name() == a[0] and np.array_equal(ctx.populations("f_next"), a[1])
        assert ctx.drain_force_log() == a[3]


# ---- 5. fp32 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
def test_fp32_mrt_against_fp64(lbm, arith):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05, mrt=(1.0, 0.25))     # tau: the default, 0.6, as in test_gpu_trt.py's fp32 comparison
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=dict(arith=arith), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        assert ctx.kernel_name().endswith("%d>" % (16 + arith))
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("mrt_fp32_vs_fp64_arith%d" % arith, err_rho=er, err_u=eu)
    print("fp32 MRT against fp64, arith %d: err_rho %.3g, err_u %.3g" % (arith, er, eu))
    assert er < 2e-5 and eu < 2e-4, (er, eu)     # the fp32 bars of tests/test_gpu_trt.py


# ---- 6. combinations on one ragged grid, a strict and a contracted register plan --------------------------------------------------------
CNX, CNY, CSTEPS, COF, CU0, CTAU = 150, 52, 60, 15, 0.05, 0.56
COMBO_PLANS = {"deep6": 0, "fast-deep7": 1}            # of PERIODIC_PLANS (row-interleaved; a periodic context runs them too): arith


def combo_mask():
    m = np.zeros((CNY, CNX), np.uint8)
    m[CNY // 2 - 3:CNY // 2 + 3, 30:37] = 1
    m[7:11, 101:104] = 1
    return m


def seam_mask():
    """A body across the seam (rows ny-3 .. ny-1 and 0 .. 2), a block mid-channel, one-cell obstacles on row 0 and row ny-1."""
    m = combo_mask()
    m[CNY - 3:, 60:66] = 1
    m[:3, 60:66] = 1
    m[0, 120] = 1
    m[CNY - 1, 133] = 1
    return m


def combo_labels():
    lab = np.zeros((CNY, CNX), np.int32)
    lab[CNY // 2 - 3:CNY // 2 + 3, 30:37] = 1
    lab[7:11, 101:104] = 2
    return lab


def combos(lbm):
    """name -> (Context keywords, reference loop, its keywords)"""
    ramp = lbm.cosine_ramp(40)
    pair = ((PRESSURE, 1.004), (PRESSURE, 0.996))
    return {
        "walls": (dict(solid=combo_mask(), walls=(FREESLIP, moving(0.04))), oracle_run, dict(mask=combo_mask(), walls=(FREESLIP, moving(0.04)))),
        "pressure-pair": (dict(solid=combo_mask(), ports=pair), ports_run, dict(mask=combo_mask(), ports=pair)),
        "periodic-y": (dict(solid=seam_mask(), periodic_y=True), periodic_run, dict(mask=seam_mask())),
        "cosine-ramp": (dict(solid=combo_mask(), inlet_schedule=(ramp, "hold")), oracle_run, dict(mask=combo_mask(), schedule=(ramp, HOLD))),
        "body-labels": (dict(bodies=combo_labels()), oracle_run, dict(mask=(combo_labels() != 0).astype(np.uint8))),
    }


COMBOS = ["walls", "pressure-pair", "periodic-y", "cosine-ramp", "body-labels"]
_combo_refs = {}


def combo_reference(lbm, combo):
    if combo not in _combo_refs:
        _, loop, kw = combos(lbm)[combo]
        run = loop(CNX, CNY, CSTEPS, COF, collide=functools.partial(mrt_collide, bulk_rate=BULK, magic=MAGIC), tau=CTAU, inlet_velocity=CU0, **kw)
        for a in (run.f_next, run.rho, run.ux, run.uy):
            a.flags.writeable = False
        _combo_refs[combo] = run
    return _combo_refs[combo]


@pytest.mark.parametrize("plan", list(COMBO_PLANS))
@pytest.mark.parametrize("combo", COMBOS)
def test_combinations_against_the_reference(lbm, combo, plan):
    ref = combo_reference(lbm, combo)
    assert ref.first_unstable == -1 and len(ref.forces) == CSTEPS // COF
    ctx_kw = combos(lbm)[combo][0]
    with lbm.Context(CNX, CNY, options=PERIODIC_PLANS[plan], tau=CTAU, inlet_velocity=CU0, mrt=MRT, **ctx_kw) as ctx:
        ctx.initialise()
        ctx.step(CSTEPS, COF)
        assert ctx.first_unstable_step() == -1
        kernel = ctx.kernel_name()
        assert kernel.startswith("k_stepc_col") and kernel.endswith(",%d>" % (16 + COMBO_PLANS[plan])), kernel
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
        if combo == "body-labels":
            blog = ctx.drain_body_force_log()
            assert sorted({b for _, b, _, _ in blog}) == [1, 2] and len(blog) == 2 * len(log)
    assert_matches_reference(COMBO_PLANS[plan], fn, macros, log, ref, U_BAR_ABS)


# ---- 7. checkpoints -------------------------------------------------------------------------------------------------------------------
def test_mrt_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    path = tmp_path / "mrt.ckpt"
    with lbm.Context(NX, NY, options=PLANS["planar-pair8-nt"], mrt=MRT, **KW) as a:
        a.initialise()
        a.step(100, 0)
        a.save_state(path)
        a.step(STEPS - 100, 0)
        assert a.first_unstable_step() == -1
        want = a.populations("f_next")
    data = open(path, "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word, then the pair
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (1024,) + MRT
    with lbm.Context(NX, NY, options=PLANS["rowil-col5-nt"], mrt=MRT, **KW) as b:      # a fresh MRT context, another kernel family
        b.initialise()
        b.load_state(path)
        b.step(STEPS - 100, 0)
        assert np.array_equal(b.populations("f_next"), want)
    with lbm.Context(NX, NY, trt_magic=MAGIC, **KW) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="written with MRT parameters"):
            c.load_state(path)
        c.step(3, 0)
        c.save_state(tmp_path / "trt.ckpt")
    with lbm.Context(NX, NY, mrt=(0.9, MAGIC), **KW) as d:
        d.initialise()
        with pytest.raises(lbm.LbmError, match="written with MRT parameters"):
            d.load_state(path)
        with pytest.raises(lbm.LbmError, match="written without a MRT parameters"):
            d.load_state(tmp_path / "trt.ckpt")
    with lbm.Context(NX, NY, **KW) as e:
        e.initialise()
        with pytest.raises(lbm.LbmError, match="written with MRT parameters"):
            e.load_state(path)


# ---- 8. the host CLI ----------------------------------------------------------------------------------------------------------------------
def test_lbm_solver_mrt_matches_the_binding(lbm, tmp_path):
    steps = 181
    pr = run_solver(["--nx", str(NX), "--ny", str(NY), "--steps", str(steps), "--output-frequency", str(OF), "--tau", str(KW["tau"]),
                     "--inlet-velocity", str(KW["inlet_velocity"]), "--cylinder-radius", str(KW["cylinder_radius"]), "--no-vtk",
                     "--mrt", "1.0,0.1875"], tmp_path)
    assert "MRT collision, bulk rate = 1, magic = 0.1875" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(NX, NY, mrt=(1.0, 0.1875), **KW) as ctx:
        ctx.initialise()
        ctx.step(steps, OF)
        assert ctx.first_unstable_step() == -1
        log = ctx.drain_force_log()
    assert [int(r[0]) for r in rows] == [t for t, _, _ in log] and len(log) == 4
    for r, (t, fx, fy) in zip(rows, log):
        for got, want in zip(map(float, r[1:3]), (fx, fy)):
            assert abs(got - want) <= 1.5e-8, (t, r)
    params = read_params(tmp_path / "simulation_params.csv")
    assert float(params["mrt_bulk_rate"]) == 1.0 and float(params["mrt_magic"]) == 0.1875
    assert abs(float(params["tau"]) - KW["tau"]) < 1e-12
