"""The outlet sponge (lbm_set_sponge, Context / Group(sponge=(width, tau_end)), lbm_solver --sponge) on the GPU.

The reference operator is sponge_collide of tests/sponge_reference.py: numpy, IEEE, BGK's strict operation order with the rate of the
cell's column, (1 / sponge_tau)[x] cast once to the element type. It replaces o.collide() in the stepwise reference loops (oracle_run,
ports_run, periodic_run); oracle/ is untouched. fp64 strict plans must match it bit for bit and contracted ones within 1e-10; fp32 strict
plans must match the float32 run bit for bit and contracted ones stay within four float32 floors of the float64 run (the rule of
tests/test_gpu_f32_oracle.py). A kernel that takes the wrong column's rate fails every bit-exact case: the rate differs from column to
column over the whole zone.

The shapes the table withholds from the sponge (collision_models, csrc/lbm_plan.hpp: tall = false, park = false): "deep" 8, the fp32
64x48 regions, and "deep" 10 / 11, the fp64 64x40 regions. No plan of tests/helpers.py PLANS pins one of them."""
import struct

import numpy as np
import pytest

from tests import f32_oracle_cases as oc
from tests.helpers import (ORACLE_PLANS, PLANS, U_BAR_ABS, assert_group_is_whole, assert_matches_reference, every_row_differs,  # noqa: F401
                           lbm_gpu, record, whole_run)
from tests.periodic_reference import periodic_run
from tests.ports_reference import PRESSURE, ports_run
from tests.reference import FREESLIP, REPEAT, oracle_run, snapshot
from tests.sponge_reference import KW, NX, NY, OF, SPONGE, STEPS, TAU_END, WIDTH, collide_of, edge_reference, read_only, reference
from tests.test_gpu_f32_oracle import FAST_PLANS, STRICT_PLANS, strict_problems
from tests.test_gpu_frames import check as check_frame
from tests.test_gpu_frames import reference_frame
from tests.test_gpu_periodic import PERIODIC_PLANS
from tests.test_gpu_probes import interpolate
from tests.test_gpu_stats import accumulate

pytestmark = pytest.mark.gpu

ENDS = (",32>", ",33>")
ALL_PLANS = list(dict.fromkeys(ORACLE_PLANS + list(PLANS)))
SITE, REG, LDS = "rowil-site-nt", "rowil-col5-nt", "rowil-deep6-nt"


def arith_of(plan):
    return int((PLANS[plan] or {}).get("arith", 0))


# ---- 1. every plan against the reference, fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ALL_PLANS)
def test_sponge_against_the_reference(lbm, plan):
    ref, plain = reference("f64"), reference("f64", False)
    assert ref.first_unstable == -1                              # precondition, on the CPU before any GPU run: stable, and not plain BGK
    assert float(np.max(np.abs(ref.f_next - plain.f_next))) > 1e-6
    with lbm.Context(NX, NY, options=PLANS[plan], sponge=SPONGE, **KW) as ctx:
        assert ctx.initialise() == ref.solid_count
        ctx.step(STEPS, OF)
        assert ctx.first_unstable_step() == ref.first_unstable
        log = ctx.drain_force_log()
        fn = ctx.populations("f_next")
        macros = ctx.macros()
        assert ctx.kernel_name().endswith(ENDS[arith_of(plan)] if plan != "auto" else ENDS), ctx.kernel_name()
        assert ctx.sponge() == SPONGE
        assert ctx.sponge_rate(NX - 1) == 1.0 / TAU_END and ctx.sponge_rate(NX - 1 - WIDTH) == 1.0 / KW["tau"]
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 2. fp32 ------------------------------------------------------------------------------------------------------------------------
def run_f32(lbm, plan):
    with lbm.Context(NX, NY, precision="f32", options=PLANS[plan], sponge=SPONGE, **KW) as ctx:
        count = ctx.initialise()
        ctx.step(STEPS, OF)
        k = ctx.kernel_name().replace(" ", "")
        assert "<float" in k and k.endswith(ENDS[arith_of(plan)]), (plan, k)
        assert ctx.sponge_rate(NX - 1) == float(np.float32(1.0 / TAU_END))
        return count, ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.first_unstable_step()


@pytest.mark.parametrize("plan", STRICT_PLANS)
def test_strict_fp32_equals_the_float32_reference(lbm, plan):
    ref = reference("f32")
    assert ref.first_unstable == -1 and np.all(np.isfinite(ref.f_next)) and ref.f_next.dtype == np.float32
    bad = strict_problems(run_f32(lbm, plan), ref)
    assert not bad, "%s: %s" % (plan, "; ".join(bad))


@pytest.mark.parametrize("plan", FAST_PLANS)
def test_contracted_fp32_within_four_floors_of_the_float64_reference(lbm, plan):
    ref = reference("f64")
    floor = oc.floors_of_runs(reference("f32"), ref)
    assert ref.first_unstable == -1 and all(v > 0.0 for v in floor)
    count, fn, macros, log, unstable = run_f32(lbm, plan)
    assert count == ref.solid_count and unstable == -1
    err = oc.errors(fn, macros, ref)
    ratio = [e / f for e, f in zip(err, floor)]
    record("sponge_f32_contracted", plan=plan, err_f=err[0], err_rho=err[1], err_u=err[2], floor_f=floor[0], floor_rho=floor[1], floor_u=floor[2])
    print("contracted fp32 sponge on %s: err / floor = %.2f (f) %.2f (rho) %.2f (u)" % ((plan,) + tuple(ratio)))
    bad = oc.contracted_problems(err, floor)
    assert not bad, "%s: %s" % (plan, "; ".join(bad))
    assert [r[0] for r in log] == [r[0] for r in ref.forces]


# ---- 3. edge shapes: strict fp64 on the register kernel and on an LDS tile ---------------------------------------------------------------
E_STEPS, E_OF = 60, 15
EDGES = [(150, 48, 1),        # only the port column
         (150, 48, 149),      # the whole domain but column 0
         (70, 48, 37),        # a zone edge inside a region, ragged nx
         (40, 48, 20),        # nx < 64: lanes without a column
         (260, 48, 130)]      # a zone wider than one region


@pytest.mark.parametrize("plan", [REG, LDS])
@pytest.mark.parametrize("nx, ny, width", EDGES)
def test_edge_shapes_against_the_reference(lbm, nx, ny, width, plan):
    ref = edge_reference(nx, ny, width, E_STEPS, E_OF)
    assert ref.first_unstable == -1 and len(ref.forces) == E_STEPS // E_OF
    with lbm.Context(nx, ny, options=PLANS[plan], sponge=(width, TAU_END), **KW) as ctx:
        assert ctx.initialise() == ref.solid_count
        ctx.step(E_STEPS, E_OF)
        assert ctx.first_unstable_step() == -1
        kernel = ctx.kernel_name()
        assert kernel.startswith("k_stepc_col" if plan == REG else "k_stepd_tile") and kernel.endswith(",32>"), kernel
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
        rates = np.array([ctx.sponge_rate(x) for x in range(nx)])
    assert np.array_equal(rates, 1.0 / lbm.sponge_tau(nx, KW["tau"], width, TAU_END))
    assert_matches_reference(plan, fn, macros, log, ref, U_BAR_ABS)


# ---- 4. combinations, one case each, strict fp64 on the register kernel -------------------------------------------------------------------
CSTEPS, COF, CU0, CTAU = 60, 15, 0.05, 0.56
CPLAN = PERIODIC_PLANS["deep6"]            # the register kernel, five iterations per launch, strict (a periodic context runs it too)
CKW = dict(tau=CTAU, inlet_velocity=CU0)


def zone_labels():
    """Body 1 upstream of the zone, body 2 a square inside it (columns 125 .. 134 of the zone's 112 .. 159)."""
    lab = np.zeros((NY, NX), np.int32)
    lab[NY // 2 - 3:NY // 2 + 3, 30:37] = 1
    lab[10:20, 125:135] = 2
    return lab


def zone_mask():
    return (zone_labels() != 0).astype(np.uint8)


def seam_zone_mask():
    """zone_mask and a body across the periodic seam, inside the zone too."""
    m = zone_mask()
    m[NY - 3:, 140:146] = 1
    m[:3, 140:146] = 1
    return m


def combos():
    """name -> (Context keywords, reference loop, its keywords)"""
    u = every_row_differs(NY, CU0)
    sched = np.random.default_rng(7).uniform(0.2, 1.0, 7)
    pair = ((PRESSURE, 1.004), (PRESSURE, 0.996))
    return {
        "body-labels": (dict(bodies=zone_labels()), oracle_run, dict(mask=zone_mask())),
        "profile-repeat-schedule": (dict(solid=zone_mask(), inlet_profile=u, inlet_schedule=(sched, "repeat")), oracle_run,
                                    dict(mask=zone_mask(), u=u, schedule=(sched, REPEAT))),
        "pressure-pair": (dict(solid=zone_mask(), ports=pair), ports_run, dict(mask=zone_mask(), ports=pair)),
        "periodic-y": (dict(solid=seam_zone_mask(), periodic_y=True), periodic_run, dict(mask=seam_zone_mask())),
        "free-slip": (dict(solid=zone_mask(), walls=(FREESLIP, FREESLIP)), oracle_run, dict(mask=zone_mask(), walls=(FREESLIP, FREESLIP))),
    }


COMBOS = ["body-labels", "profile-repeat-schedule", "pressure-pair", "periodic-y", "free-slip"]
_combo_refs = {}


def combo_reference(combo, steps=CSTEPS):
    if (combo, steps) not in _combo_refs:
        _, loop, kw = combos()[combo]
        _combo_refs[combo, steps] = read_only(loop(NX, NY, steps, COF, collide=collide_of(), **CKW, **kw))
    return _combo_refs[combo, steps]


@pytest.mark.parametrize("combo", COMBOS)
def test_combinations_against_the_reference(lbm, combo):
    ref = combo_reference(combo)
    assert ref.first_unstable == -1 and len(ref.forces) == CSTEPS // COF
    with lbm.Context(NX, NY, options=CPLAN, sponge=SPONGE, **CKW, **combos()[combo][0]) as ctx:
        assert ctx.initialise() == ref.solid_count
        ctx.step(CSTEPS, COF)
        assert ctx.first_unstable_step() == -1
        kernel = ctx.kernel_name()
        assert kernel.startswith("k_stepc_col") and kernel.endswith(",32>"), kernel
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
        blog = ctx.drain_body_force_log() if combo == "body-labels" else None
    assert_matches_reference(0, fn, macros, log, ref, U_BAR_ABS)
    if blog is not None:          # forces per body: both bodies at every output, and the two add up to the force log's row
        assert sorted({b for _, b, _, _ in blog}) == [1, 2] and len(blog) == 2 * len(log)
        for t, fx, fy in log:
            bx = sum(r[2] for r in blog if r[0] == t)
            by = sum(r[3] for r in blog if r[0] == t)
            assert abs(bx - fx) <= 1e-10 * max(1.0, abs(fx)) and abs(by - fy) <= 1e-10 * max(1.0, abs(fy)), (t, bx, fx, by, fy)
        assert any(abs(r[2]) > 1e-6 for r in blog if r[1] == 2)          # the body inside the zone feels the flow


def test_two_strips_are_the_one_strip_run(lbm):
    kw = dict(sponge=SPONGE, solid=zone_mask(), **CKW)
    w = whole_run(lbm, NX, NY, REG, CSTEPS, COF, **kw)
    with lbm.Group(NX, NY, 2, options=PLANS[REG], **kw) as g:
        g.initialise()
        g.step(CSTEPS, COF)
        assert g.first_unstable_step() == -1
        assert all(c.kernel_name().endswith(",32>") and c.sponge() == SPONGE and c.local_ny == NY // 2 for c in g.ctxs)
        assert all(c.sponge_rate(NX - 1) == 1.0 / TAU_END for c in g.ctxs)          # strips cut rows: every strip holds the whole table
        assert_group_is_whole(g, w)


def test_checkpoint_saved_mid_run_and_resumed(lbm, tmp_path):
    path = tmp_path / "sponge.ckpt"
    ref = reference("f64")
    with lbm.Context(NX, NY, options=PLANS["planar-pair8-nt"], sponge=SPONGE, **KW) as a:
        a.initialise()
        a.step(100, 0)
        a.save_state(path)
    data = open(path, "rb").read()
    # the fixed header is 72 bytes (magic word, six ints, five doubles); then the flag word, then the pair
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (2048, float(WIDTH), TAU_END)
    with lbm.Context(NX, NY, options=PLANS[REG], sponge=SPONGE, **KW) as b:      # a fresh sponge context, another kernel family
        b.initialise()
        b.load_state(path)
        b.step(STEPS - 100, 0)
        assert b.first_unstable_step() == -1 and np.array_equal(b.populations("f_next"), ref.f_next)
    for other, text in ((dict(sponge=(WIDTH - 1, TAU_END)), "written with sponge"), (dict(sponge=(WIDTH, 1.25)), "written with sponge"),
                        ({}, r"written with sponge \(width, tau_end\) = \(48, 1\.5\); this context has none"),
                        (dict(mrt=(1.0, 0.1875)), "written with sponge")):
        with lbm.Context(NX, NY, options=PLANS[SITE], **KW, **other) as c:
            c.initialise()
            with pytest.raises(lbm.LbmError, match=text):
                c.load_state(path)
            if not other:
                c.save_state(tmp_path / "bgk.ckpt")
    with lbm.Context(NX, NY, options=PLANS[SITE], sponge=SPONGE, **KW) as d:
        d.initialise()
        with pytest.raises(lbm.LbmError, match="written without a sponge"):
            d.load_state(tmp_path / "bgk.ckpt")


def test_statistics_frames_and_probes_are_those_of_the_reference_snapshot(lbm):
    """The samples of output iteration t describe the state macros() reports after t + 1 iterations: the snapshot of the reference run of
    that length (tests/reference.py snapshot), which a strict fp64 plan reproduces bit for bit."""
    k = 4
    pts = [t for t in range(CSTEPS) if t % COF == 0]
    xy = np.array([(5.0, 5.0), (NX - 1.0, 9.5), (NX - 1.25, 20.0), (120.5, 30.25), (111.0, 24.0), (112.75, 0.0), (140.0, NY - 1.0), (63.5, 15.5)])
    snaps = {t: snapshot(combo_reference("free-slip", t + 1)) for t in pts}
    with lbm.Context(NX, NY, options=CPLAN, sponge=SPONGE, **CKW, **combos()["free-slip"][0]) as ctx:
        ctx.initialise()
        ctx.stats_begin(0)
        ctx.frames_begin(k, 8)
        ctx.probes_begin(xy, 8)
        ctx.step(CSTEPS, COF)
        assert ctx.first_unstable_step() == -1 and ctx.kernel_name().endswith(",32>")
        sums, n = ctx.stats_sums(), ctx.stats_samples()
        frames = ctx.drain_frames()
        ts, vals = ctx.drain_probes()
    S = np.zeros((6, NY, NX))
    for t in pts:
        S = accumulate(S, snaps[t])
    assert n == len(pts) and np.array_equal(sums, S)
    assert [t for t, _ in frames] == pts
    for t, f in frames:
        check_frame(f, reference_frame(snaps[t], k), "sponge frame of t = %d" % t)
    assert ts.tolist() == pts and vals.shape == (len(pts), len(xy), 3)
    for j, t in enumerate(pts):
        assert np.array_equal(vals[j], interpolate(snaps[t], xy)), t


# ---- 5. width = 0 is BGK ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", REG, "planar-fuse3-8", "fast-rowil-col6", LDS, "planar-site"])
def test_width_zero_after_a_nonzero_call_is_bgk(lbm, plan):
    nx, ny, steps, of = 200, 64, 97, 30
    kw = dict(tau=0.55, inlet_velocity=0.06)
    with lbm.Context(nx, ny, options=PLANS[plan], **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        a = (ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log())
        assert ctx.sponge() == (0, 0.0) and ctx.sponge_rate(nx - 1) == 1.0 / kw["tau"]
    with lbm.Context(nx, ny, options=PLANS[plan], sponge=(48, 1.5), **kw) as ctx:     # set, then cleared
        ctx.set_sponge(0, 1.5)
        assert ctx.sponge() == (0, 0.0)
        ctx.initialise()
        ctx.step(steps, of)
        b = (ctx.kernel_name(), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log())
        assert ctx.sponge_rate(nx - 1) == 1.0 / kw["tau"]
    assert a[0] == b[0] and a[0].endswith((",0>", ",1>"))
    assert np.array_equal(a[1], b[1]) and a[3] == b[3]
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(x, y)


def test_withheld_shapes_are_refused(lbm):
    noun = "no outlet sponge kernel"
    with lbm.Context(256, 64, precision="f32", sponge=SPONGE) as ctx:                              # tall: the fp32 64x48 regions
        with pytest.raises(lbm.LbmError, match=noun):
            ctx.set_option("deep", 8)
    for deep in (10, 11):                                                                        # park: the fp64 64x40 regions
        with lbm.Context(256, 96, options=dict(tune=0, arith=1, deep=deep)) as ctx:
            with pytest.raises(lbm.LbmError, match=r"deep %d \(64x40 regions in registers\) has %s" % (deep, noun)):
                ctx.set_sponge(*SPONGE)
