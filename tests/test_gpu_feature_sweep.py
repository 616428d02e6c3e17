"""The features crossed with each other, with every kernel family and with ragged grids (the cases of tests/feature_cases.py).

Every feature has a test module of its own that holds the GPU to the stepwise reference at one friendly lattice, 160x48. Here the
collision models (BGK, Smagorinsky LES, TRT, BGK under a driving force) meet masks, inlet profiles and schedules, the wall kinds, call
sequences, strips of odd heights and checkpoints on grids narrower than a tile, lower than a region and with partial last bands and
columns, and the register kernel's LEAN path (interior tiles: almost every tile of a real grid) is held to the reference for every model.

fp64: against tests/reference.py oracle_run with the model's operator, at the bars of helpers.assert_matches_reference: strict plans
f_next bit for bit and rho within 1e-14, contracted ones within 1e-10, force rows within 1e-10. fp32: bit for bit against the same
context stepped at one iteration per launch in the same arithmetic, as tests/test_gpu_random.py does, and those single iterations
against the reference: in strict arithmetic bit for bit against the same loop in float32 (feature_cases.reference32_of: f_next, the
macro snapshot, the first unstable iteration), in contracted arithmetic against the fp64 reference within four float32 floors of the case
(tests/f32_oracle_cases.py contracted_problems). Every run must name the kernel of its model and arithmetic mode, so no case can pass
on another model's kernel."""
import functools

import numpy as np
import pytest

from tests import f32_oracle_cases as oc
from tests import feature_cases as fc
from tests.helpers import PLANS, U_BAR_ABS, assert_forces_match, assert_matches_reference, lbm_gpu, record, where  # noqa: F401
from tests.reference import snapshot

pytestmark = pytest.mark.gpu

ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)             # one iteration per launch


def make(lbm, case, plan=None):
    kw, opts = fc.context_kw(case), fc.options_of(case, plan)
    if case.strips > 1:
        return lbm.Group(case.nx, case.ny, case.strips, options=opts, **kw)
    return lbm.Context(case.nx, case.ny, options=opts, **kw)


def assert_kernel(ctx, model, plan):
    """Every member runs the kernel of the model in the plan's arithmetic mode: <.., Arith> with 0 / 1 BGK, 2 / 3 LES, 4 / 5 TRT, 8 / 9 forced."""
    want = ",%d>" % (fc.MODEL_BASE[model] | fc.contracted(plan))
    for c in getattr(ctx, "ctxs", [ctx]):
        assert c.kernel_name().endswith(want), "kernel %s, expected one ending in %s" % (c.kernel_name(), want)


def bar_key(plan):
    """What helpers.strict takes: the plan's name, or for a pinned plan that is no key of PLANS its arithmetic mode."""
    return plan if plan in PLANS else fc.contracted(plan)


def record_contracted(name, plan, fn, macros, ref, **what):
    if fc.contracted(plan):
        rho, ux, uy = macros
        record(name, plan=plan, family=fc.family(plan), err_f=float(np.max(np.abs(fn - ref.f_next)) / np.max(np.abs(ref.f_next))),
               err_rho=float(np.max(np.abs(rho - ref.rho))),
               err_u=max(float(np.max(np.abs(ux - ref.ux))), float(np.max(np.abs(uy - ref.uy)))), **what)


# ---- 1. fp64: the seeded cases against the reference, a third of the single contexts through a checkpoint ---------------------------
def run_fp64_case(lbm, case, tmp_path):
    ref = fc.reference_of(case)
    calls = fc.issued_calls(case)
    # (a reference that went unstable defines only the iteration it reports: such a case runs on one context)
    handover = case.ckpt_plan is not None and ref.first_unstable == -1
    first = calls[0] if handover else 0
    plan = case.plan
    if handover:
        with make(lbm, case) as a:
            assert a.initialise() == ref.solid_count
            a.step(first, case.of)
            assert_kernel(a, case.model, plan)
            assert a.first_unstable_step() == -1
            assert_forces_match(a.drain_force_log(), [r for r in ref.forces if r[0] < first], "before the checkpoint")
            a.save_state(tmp_path / "handover.ckpt")
        plan, calls = case.ckpt_plan, calls[1:]
        ref = ref._replace(forces=[r for r in ref.forces if r[0] >= first])
    with make(lbm, case, plan) as ctx:
        assert ctx.initialise() == ref.solid_count
        if handover:
            ctx.load_state(tmp_path / "handover.ckpt")
        for n in calls:
            ctx.step(n, case.of)
        assert_kernel(ctx, case.model, plan)
        assert ctx.first_unstable_step() == ref.first_unstable
        if ref.first_unstable != -1:
            return
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
    record_contracted("feature_sweep_fp64", plan, fn, macros, ref, case=case.k, model=case.model, strips=case.strips)
    assert_matches_reference(bar_key(plan), fn, macros, log, ref, U_BAR_ABS)


@pytest.mark.parametrize("case", fc.fp64_cases(), ids=fc.case_id)
def test_fp64_case_matches_the_reference(lbm, case, tmp_path):
    try:
        run_fp64_case(lbm, case, tmp_path)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, case)) from e


# ---- 2. fp32: the seeded cases against one launch per iteration ----------------------------------------------------------------------
def run_fp32_case(lbm, case):
    with lbm.Context(case.nx, case.ny, options=dict(ONE, arith=fc.contracted(case.plan)), **fc.context_kw(case)) as one:
        count = one.initialise()
        for n in case.calls:
            one.step(n, case.of)
        assert one.kernel_name().startswith("k_step_site<float") and one.kernel_name().endswith(
            ",%d>" % (fc.MODEL_BASE[case.model] | fc.contracted(case.plan))), one.kernel_name()
        r_bad = one.first_unstable_step()
        if r_bad == -1:
            r_fn, r_macros, r_log = one.populations("f_next"), one.macros(), one.drain_force_log()
    # the single iterations themselves against the reference: what every plan is held to below is then held to ground truth
    if not fc.contracted(case.plan):
        ref = fc.reference32_of(case)
        assert count == ref.solid_count and r_bad == ref.first_unstable, (count, ref.solid_count, r_bad, ref.first_unstable)
        if r_bad == -1:
            want = ref.f_next.astype(np.float64)
            assert np.array_equal(r_fn, want), "the single iterations' f_next is not the float32 reference's bit for bit: " + where(r_fn, want)
            for got, want in zip(r_macros, snapshot(ref)):
                assert np.array_equal(got, want.astype(np.float64)), "the single iterations' macros are not the float32 reference's snapshot"
            assert_forces_match(r_log, ref.forces, "single iterations")
    elif fc.reference_of(case).first_unstable == -1:
        ref = fc.reference_of(case)
        assert count == ref.solid_count and r_bad == -1, (count, ref.solid_count, r_bad)
        err, floor = oc.errors(r_fn, r_macros, ref), oc.floors_of_runs(fc.reference32_of(case), ref)
        record("f32_oracle_sweep_contracted", case=case.k, model=case.model, steps=fc.steps_of(case), err_f=err[0], err_rho=err[1], err_u=err[2],
               floor_f=floor[0], floor_rho=floor[1], floor_u=floor[2])
        bad = oc.contracted_problems(err, floor)
        assert not bad, "the single iterations against the float64 reference: " + "; ".join(bad)
    with make(lbm, case) as ctx:
        assert ctx.initialise() == count
        for n in fc.issued_calls(case):
            ctx.step(n, case.of)
        assert_kernel(ctx, case.model, case.plan)
        assert ctx.first_unstable_step() == r_bad
        if r_bad != -1:
            return
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
    assert np.all(np.isfinite(r_fn)) and np.array_equal(fn, r_fn), "f_next is not the single iterations' bit for bit: " + where(fn, r_fn)
    for got, want in zip(macros, r_macros):
        assert np.array_equal(got, want), "macros differ"
    assert [r[0] for r in log] == [r[0] for r in r_log]
    for (t, fx, fy), (_, wx, wy) in zip(log, r_log):
        if case.strips == 1:
            assert fx == wx and fy == wy, (t, fx, fy, wx, wy)
        else:       # (the strips' partial sums are added in another order)
            assert abs(fx - wx) <= 1e-5 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-5 * max(1.0, abs(wy)), (t, fx, fy, wx, wy)


@pytest.mark.parametrize("case", fc.fp32_cases(), ids=fc.case_id)
def test_fp32_case_equals_single_iterations(lbm, case):
    try:
        run_fp32_case(lbm, case)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, case)) from e


# ---- 3. the LEAN path of every model against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("plan", fc.LEAN_PLANS)
@pytest.mark.parametrize("model", list(fc.LEAN_MODELS))
def test_lean_tiles_against_the_reference(lbm, model, plan):
    ref = fc.lean_reference(model)
    assert ref.first_unstable == -1 and [r[0] for r in ref.forces] == [0, 16]
    with lbm.Context(fc.LEAN_NX, fc.LEAN_NY, options=fc.plan_options(plan), **fc.lean_kw(model)) as ctx:
        assert ctx.initialise() == ref.solid_count
        ctx.step(fc.LEAN_STEPS, fc.LEAN_OF)
        assert_kernel(ctx, model, plan)
        assert ctx.first_unstable_step() == -1
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
    record_contracted("feature_sweep_lean", plan, fn, macros, ref, model=model)
    assert_matches_reference(bar_key(plan), fn, macros, log, ref, U_BAR_ABS)


@functools.lru_cache(maxsize=None)
def lean_single_iterations(lbm, model, arith):
    """The fp32 lean-tile case of a model at one iteration per launch: what every fp32 plan of that arithmetic mode must equal."""
    with lbm.Context(fc.LEAN_NX, fc.LEAN_NY_F32, precision="f32", options=dict(ONE, arith=arith), **fc.lean_kw(model)) as one:
        count = one.initialise()
        one.step(fc.LEAN_STEPS, fc.LEAN_OF)
        assert one.kernel_name().startswith("k_step_site<float") and one.first_unstable_step() == -1
        return count, one.populations("f_next"), one.macros(), one.drain_force_log()


@pytest.mark.parametrize("model,plan", fc.LEAN_PLANS_F32, ids=lambda v: v)
def test_lean_tiles_fp32_equal_single_iterations(lbm, model, plan):
    count, r_fn, r_macros, r_log = lean_single_iterations(lbm, model, fc.contracted(plan))
    assert len(r_log) == 2 and np.all(np.isfinite(r_fn))
    with lbm.Context(fc.LEAN_NX, fc.LEAN_NY_F32, precision="f32", options=fc.plan_options(plan), **fc.lean_kw(model)) as ctx:
        assert ctx.initialise() == count
        ctx.step(fc.LEAN_STEPS, fc.LEAN_OF)
        assert_kernel(ctx, model, plan)
        assert ctx.kernel_name().replace(" ", "").startswith("k_stepc_col<float,"), ctx.kernel_name()
        assert ctx.first_unstable_step() == -1
        fn = ctx.populations("f_next")
        assert np.array_equal(fn, r_fn), "f_next is not the single iterations' bit for bit: " + where(fn, r_fn)
        for got, want in zip(ctx.macros(), r_macros):
            assert np.array_equal(got, want)
        assert ctx.drain_force_log() == r_log
