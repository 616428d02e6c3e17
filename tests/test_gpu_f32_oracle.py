"""The fp32 kernels against a float32 reference of full precision (the cases of tests/f32_oracle_cases.py).

Strict fp32 arithmetic is IEEE float32 one operation at a time: the collision's constants are T(double literal), its two divisions
and its square roots are correctly rounded, nothing is contracted, and every value the host forms is formed in double and cast once.
tests/reference.py with dtype=np.float32 (on tests/numpy_oracle.py) evaluates the same operations on float32 arrays, so a strict fp32
plan must give its f_next, ghost cells included, BIT FOR BIT, its macros must be tests/reference.py snapshot of that run bit for bit,
and the first unstable iteration and the solid count must be the reference's; the force rows are fp64 sums of the same addends in another
order and stay at 1e-10 max(1, |F|). One wrong cell, one constant formed in double, one cast in the wrong place fails it. The fp64
site plan runs beside it as a control: it equals the float64 reference to the bit, and the fp32 result is not that result cast.

Contracted fp32 arithmetic (one v_rcp_f32 with a Newton step, FMAs) cannot be transcribed. It is another float32 rounding history of the
same formulas, and is held to the float64 reference at four times the case's float32 floor (f32_oracle_cases.floors: the float32
reference against the float64 one), in f_next, rho and u; every measured ratio is recorded. tests/test_f32_reference_cpu.py shows on the
CPU that four floors are below the bars (2e-5 on rho, 2e-4 on u) the fp32 kernels are held to elsewhere."""
import numpy as np
import pytest

from tests import f32_oracle_cases as oc
from tests import feature_cases as fc
from tests.helpers import PLANS, force_problems, lbm_gpu, record, where  # noqa: F401
from tests.reference import snapshot
from tests.test_gpu_periodic import PERIODIC_PLANS

pytestmark = pytest.mark.gpu

STRICT_PLANS = ["rowil-site-nt", "planar-pair8-nt", "planar-fuse3-8", "rowil-fuse4-nt-xcd", "rowil-deep6-nt", "planar-deep7-alt", "rowil-deep8-nt",
                "rowil-col5-nt", "planar-col6-alt", "rowil-col7-alt"]
FAST_PLANS = ["fast-site", "fast-rowil-col6", "fast-rowil-col7", "fast-rowil-deep7"]
SITE, REG = "rowil-site-nt", "rowil-col5-nt"


def first_difference(got, want):
    """helpers.where and the population: the first cell of two ghost-inclusive arrays that differs, for the failure message."""
    d = np.argwhere(got != want)
    if not len(d):
        return "equal"
    y, x, i = d[0]
    return "%s; there population %d is %.9g, the reference's %.9g" % (where(got, want), i, got[y, x, i], want[y, x, i])


def options_of(plan):
    return PERIODIC_PLANS[plan] if plan in PERIODIC_PLANS else fc.plan_options(plan)


def arith_of(plan):
    return int(options_of(plan).get("arith", 0))


def run_case(lbm, name, plan, precision="f32", strips=1):
    """(solid count, f_next, macros, force log, first unstable iteration) of the case's context (strips > 1: group) on a plan; the
    kernel must be the model's, in the plan's arithmetic mode and the precision asked for."""
    c = oc.CASES[name]
    kw = dict(c.ctx_kw, precision=precision, options=options_of(plan))
    with (lbm.Group(c.nx, c.ny, strips, **kw) if strips > 1 else lbm.Context(c.nx, c.ny, **kw)) as ctx:
        count = ctx.initialise()
        for n, of in c.calls:
            ctx.step(n, of)
        for m in getattr(ctx, "ctxs", [ctx]):
            k = m.kernel_name().replace(" ", "")
            assert ("<float" if precision == "f32" else "<double") in k and k.endswith(",%d>" % (oc.MODEL_BASE[c.model] | arith_of(plan))), (plan, k)
        return count, ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.first_unstable_step()


def strict_problems(run, ref):
    """What of a strict run misses the reference run of its precision: everything but the forces bit for bit."""
    count, fn, macros, log, bad = run
    out = []
    if count != ref.solid_count:
        out.append("%d solid cells, the reference %d" % (count, ref.solid_count))
    if bad != ref.first_unstable:
        out.append("first unstable iteration %d, the reference's %d" % (bad, ref.first_unstable))
    want = ref.f_next.astype(np.float64)
    if not np.array_equal(fn, want):
        out.append("f_next is not the reference's bit for bit: " + first_difference(fn, want))
    for k, got, want in zip(("rho", "ux", "uy"), macros, snapshot(ref)):
        if not np.array_equal(got, want.astype(np.float64)):
            y, x = np.argwhere(got != want)[0]
            out.append("%s is not the snapshot of the reference bit for bit: first at (x, y) = (%d, %d), %.9g against %.9g, %d cells differ"
                       % (k, x, y, got[y, x], want[y, x], int(np.sum(got != want))))
    return out + force_problems(log, ref.forces)


def assert_strict(lbm, name, plan, precision="f32", strips=1):
    ref = oc.reference(name, precision)
    assert ref.first_unstable == -1 and np.all(np.isfinite(ref.f_next))          # on the CPU, before any GPU run
    bad = strict_problems(run_case(lbm, name, plan, precision, strips), ref)
    assert not bad, "%s on %s%s: %s" % (name, plan, " in %d strips" % strips if strips > 1 else "", "; ".join(bad))


# ---- a. strict fp32 against the float32 reference, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("plan", STRICT_PLANS)
@pytest.mark.parametrize("model", list(oc.MODELS))
def test_strict_families_and_models_equal_the_float32_reference(lbm, model, plan):
    assert_strict(lbm, oc.FAMILIES[model], plan)


@pytest.mark.parametrize("model,plan", [(m, p) for m in oc.MODELS for p in (REG, "rowil-col7-alt")] + [("bgk", "tall-f32")], ids=lambda v: v)
def test_strict_lean_tiles_equal_the_float32_reference(lbm, model, plan):
    assert_strict(lbm, oc.LEAN[model], plan)


def test_strict_tall_regions_equal_the_float32_reference(lbm):
    assert_strict(lbm, oc.FAMILIES["bgk"], "tall-f32")


@pytest.mark.parametrize("plan", [SITE, REG])
@pytest.mark.parametrize("name", oc.FEATURES)
def test_strict_features_equal_the_float32_reference(lbm, name, plan):
    assert_strict(lbm, name, plan)


@pytest.mark.parametrize("plan", [k for k in PERIODIC_PLANS if not PERIODIC_PLANS[k].get("arith")])
def test_strict_periodic_y_equals_the_float32_reference(lbm, plan):
    assert_strict(lbm, oc.PERIODIC, plan)


@pytest.mark.parametrize("plan", [REG, SITE])
@pytest.mark.parametrize("strips", [2, 3])
def test_strict_strips_equal_the_float32_reference(lbm, strips, plan):
    assert_strict(lbm, oc.FAMILIES["bgk"], plan, strips=strips)


@pytest.mark.parametrize("model", list(oc.MODELS))
def test_one_step_from_the_references_state(lbm, model):
    """The float32 reference's f_current after ten iterations, loaded into a site-plan context, and one step: no error accumulates, so
    a difference names the first wrong cell and population of one collision, one streaming step and one boundary step."""
    name = oc.FAMILIES[model]
    c = oc.CASES[name]
    c10 = oc.LOOPS[c.loop](c.nx, c.ny, 10, 0, dtype=np.float32, keep_f_current=True, **c.ref_kw)[1]
    ref11, c11 = oc.LOOPS[c.loop](c.nx, c.ny, 11, 0, dtype=np.float32, keep_f_current=True, **c.ref_kw)
    assert ref11.first_unstable == -1 and c10.dtype == np.float32
    with lbm.Context(c.nx, c.ny, precision="f32", options=PLANS[SITE], **c.ctx_kw) as ctx:
        assert ctx.initialise() == ref11.solid_count
        ctx.set_f_current(c10)
        ctx.step(1, 0)
        assert ctx.kernel_name().startswith("k_step_site<float") and ctx.first_unstable_step() == -1
        fn, fcur, macros = ctx.populations("f_next"), ctx.populations("f_current"), ctx.macros()
    want = ref11.f_next.astype(np.float64)
    assert np.array_equal(fn, want), "the collision of the loaded state: " + first_difference(fn, want)
    got, want = fcur[1:-1, 1:-1], c11.astype(np.float64)[1:-1, 1:-1]
    assert np.array_equal(got, want), "streaming and boundaries behind it: " + first_difference(np.pad(got, ((1, 1), (1, 1), (0, 0))),
                                                                                                  np.pad(want, ((1, 1), (1, 1), (0, 0))))
    for k, a, b in zip(("rho", "ux", "uy"), macros, snapshot(ref11)):
        assert np.array_equal(a, b.astype(np.float64)), k


# ---- b. the control: fp64 on the same case equals the float64 reference, and fp32 is not fp64 cast ---------------------------------------
def test_fp64_control_and_fp32_is_not_fp64_cast(lbm):
    name = oc.FAMILIES["bgk"]
    ref64 = oc.reference(name, "f64")
    run64 = run_case(lbm, name, SITE, "f64")
    bad = strict_problems(run64, ref64)                                 # (f_next and the snapshot bit for bit in fp64 too)
    assert not bad, "; ".join(bad)
    run32 = run_case(lbm, name, SITE)
    cast = run64[1].astype(np.float32).astype(np.float64)
    differ = int(np.sum(run32[1] != cast))
    assert differ > cast.size // 10, "%d of %d values of the fp32 run differ from the fp64 run cast to float32" % (differ, cast.size)


# ---- c. contracted fp32 against the float64 reference, at four float32 floors -----------------------------------------------------------
def assert_contracted(lbm, name, plan):
    ref, floor = oc.reference(name, "f64"), oc.floors(name)
    assert ref.first_unstable == -1 and all(v > 0.0 for v in floor)
    count, fn, macros, log, unstable = run_case(lbm, name, plan)
    assert count == ref.solid_count and unstable == -1
    err = oc.errors(fn, macros, ref)
    ratio = [e / f for e, f in zip(err, floor)]
    bad = oc.contracted_problems(err, floor)
    record("f32_oracle_contracted", case=name, plan=plan, err_f=err[0], err_rho=err[1], err_u=err[2], floor_f=floor[0], floor_rho=floor[1],
           floor_u=floor[2], ratio_f=ratio[0], ratio_rho=ratio[1], ratio_u=ratio[2])
    print("contracted %s on %s: err / floor = %.2f (f) %.2f (rho) %.2f (u)" % ((name, plan) + tuple(ratio)))
    assert not bad, "%s on %s: %s" % (name, plan, "; ".join(bad))
    assert [r[0] for r in log] == [r[0] for r in ref.forces]


@pytest.mark.parametrize("plan", FAST_PLANS)
@pytest.mark.parametrize("model", list(oc.MODELS))
@pytest.mark.parametrize("group", ["families", "lean"])
def test_contracted_fp32_within_four_floors_of_the_float64_reference(lbm, group, model, plan):
    assert_contracted(lbm, (oc.FAMILIES if group == "families" else oc.LEAN)[model], plan)


@pytest.mark.parametrize("group", ["families", "lean"])
def test_contracted_tall_regions_within_four_floors(lbm, group):
    assert_contracted(lbm, (oc.FAMILIES if group == "families" else oc.LEAN)["bgk"], "tall-f32-fast")
