"""Periodic y, the two ports and the MRT collision crossed with the other features, with every kernel family a strip may run and
with ragged grids (the cases of tests/feature_cases2.py): the second generation of tests/test_gpu_feature_sweep.py.

Each of the three has a test module of its own that holds the GPU to its reference on friendly lattices (200x72 and 192x48, 130x70,
160x48). Here they meet lattices from two columns and twelve rows up, random masks, profiles and schedules, rings and walled groups of
unequal strips with one of exactly twelve rows, call sequences and checkpoints handed to another family; and the smallest periodic
lattices (ny below the pad of sixteen rows, where the wrapped tables wrap more than once; nx narrower than a tile) run every strip plan.

The reference of every case is tests/periodic_reference.py periodic_run, at the bars of the first sweep. fp64: strict plans f_next bit
for bit, contracted ones within 1e-10, force rows within 1e-10 (helpers.assert_matches_reference); a group against the lone context of
its plan, fields bit for bit and force rows at helpers.assert_group_is_whole's 1e-13. fp32: bit for bit against the same context at one
iteration per launch in the same arithmetic, and those single iterations against the reference: strict bit for bit against the float32
loop, contracted within four float32 floors of the float64 one. Every run must name the kernel of its model and arithmetic mode."""
import functools

import numpy as np
import pytest

from tests import f32_oracle_cases as oc
from tests import feature_cases2 as f2
from tests.helpers import U_BAR_ABS, assert_forces_match, assert_matches_reference, force_problems, lbm_gpu, record, where  # noqa: F401
from tests.reference import snapshot
from tests.test_gpu_periodic import PERIODIC_PLANS

pytestmark = pytest.mark.gpu

ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)             # one iteration per launch


def make(lbm, case, plan=None, lone=False):
    """The case's Group (peer copies, every strip on device 0) or Context; lone: the one context a group is held to, on the group's
    plan, layout and launch order."""
    kw, opts = f2.context_kw(case), f2.options_of(case, plan)
    if f2.grouped(case) and not lone:
        bounds = f2.bounds_of(case)
        return lbm.Group(case.nx, case.ny, bounds, devices=[0] * len(bounds), transport="peer", options=opts, **kw)
    if f2.grouped(case):
        opts = dict(f2.plan_options(case.plan if plan is None else plan, case.periodic), trailing_pair=case.trailing_pair, layout=1, alternate=0)
    return lbm.Context(case.nx, case.ny, options=opts, **kw)


def assert_kernel(ctx, case, plan):
    """Every member runs the kernel of the model in the plan's arithmetic mode: <.., Arith> with 0 / 1 BGK .. 16 / 17 MRT."""
    want = ",%d>" % (f2.MODEL_BASE[case.model] | f2.contracted(plan, case.periodic))
    for c in getattr(ctx, "ctxs", [ctx]):
        assert c.kernel_name().endswith(want), "kernel %s, expected one ending in %s" % (c.kernel_name(), want)
        assert bool(c.periodic_y()) == bool(case.periodic)


def interior(case, a):
    """What a ring of strips is compared on: the strips' rows (the lone context's ghost rows hold the wrapped rows)."""
    return a[1:-1] if case.periodic else a


def assert_group_is_lone(case, fn, macros, log, lone):
    l_fn, l_macros, l_log = lone
    for u, v in zip(macros, l_macros):
        assert np.array_equal(u, v), "a group's macros are not the lone context's"
    assert np.array_equal(interior(case, fn), interior(case, l_fn)), "a group's f_next is not the lone context's: " + where(fn, l_fn)
    assert [r[0] for r in log] == [r[0] for r in l_log]
    for (t, fx, fy), (_, wx, wy) in zip(log, l_log):                 # (assert_group_is_whole's bar: sums in strip order)
        assert abs(fx - wx) <= 1e-13 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-13 * max(1.0, abs(wy)), (t, fx, fy, wx, wy)


def record_contracted(name, case, plan, fn, macros, ref, **what):
    if f2.contracted(plan, case.periodic):
        rho, ux, uy = macros
        record(name, plan=plan, family=f2.family(plan, case.periodic), periodic=case.periodic,
               err_f=float(np.max(np.abs(fn - ref.f_next)) / np.max(np.abs(ref.f_next))), err_rho=float(np.max(np.abs(rho - ref.rho))),
               err_u=max(float(np.max(np.abs(ux - ref.ux))), float(np.max(np.abs(uy - ref.uy)))), **what)


# ---- 1. fp64: the seeded cases against the reference ------------------------------------------------------------------------------------
def run_fp64_case(lbm, case, tmp_path):
    ref = f2.reference_of(case)
    calls = f2.issued_calls(case)
    # (a reference that went unstable defines only the iteration it reports: such a case runs on one context)
    handover = case.ckpt_plan is not None and ref.first_unstable == -1
    first = calls[0] if handover else 0
    plan = case.plan
    if handover:
        with make(lbm, case) as a:
            assert a.initialise() == ref.solid_count
            a.step(first, case.of)
            assert_kernel(a, case, plan)
            assert a.first_unstable_step() == -1
            assert_forces_match(a.drain_force_log(), [r for r in ref.forces if r[0] < first], "before the checkpoint")
            a.save_state(tmp_path / "handover.ckpt")
        plan, calls = case.ckpt_plan, calls[1:]
        ref = ref._replace(forces=[r for r in ref.forces if r[0] >= first])
    with make(lbm, case, plan, lone=True) as ctx:
        assert ctx.initialise() == ref.solid_count
        if handover:
            ctx.load_state(tmp_path / "handover.ckpt")
        for n in calls:
            ctx.step(n, case.of)
        assert_kernel(ctx, case, plan)
        assert ctx.first_unstable_step() == ref.first_unstable
        if ref.first_unstable == -1:
            fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
    if f2.grouped(case):
        with make(lbm, case) as g:
            assert g.initialise() == ref.solid_count
            for n in calls:
                g.step(n, case.of)
            assert_kernel(g, case, plan)
            assert g.first_unstable_step() == ref.first_unstable
            if ref.first_unstable == -1:
                assert_group_is_lone(case, g.populations("f_next"), g.macros(), g.drain_force_log(), (fn, macros, log))
    if ref.first_unstable != -1:
        return
    record_contracted("feature_sweep2_fp64", case, plan, fn, macros, ref, k=case.k, model=case.model, strips=len(f2.bounds_of(case)) if f2.grouped(case) else 1)
    assert_matches_reference(f2.contracted(plan, case.periodic), fn, macros, log, ref, U_BAR_ABS)


@pytest.mark.parametrize("case", f2.fp64_cases(), ids=f2.case_id)
def test_fp64_case_matches_the_reference(lbm, case, tmp_path):
    try:
        run_fp64_case(lbm, case, tmp_path)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, case)) from e


# ---- 2. fp32: the seeded cases against one launch per iteration, and those against the reference ----------------------------------------
def run_fp32_case(lbm, case):
    arith = f2.contracted(case.plan, case.periodic)
    with lbm.Context(case.nx, case.ny, options=dict(ONE, arith=arith), **f2.context_kw(case)) as one:
        count = one.initialise()
        for n in case.calls:
            one.step(n, case.of)
        assert one.kernel_name().startswith("k_step_site<float") and one.kernel_name().endswith(",%d>" % (f2.MODEL_BASE[case.model] | arith)), \
            one.kernel_name()
        r_bad = one.first_unstable_step()
        if r_bad == -1:
            r_fn, r_macros, r_log = one.populations("f_next"), one.macros(), one.drain_force_log()
    if not arith:
        ref = f2.reference32_of(case)
        assert count == ref.solid_count and r_bad == ref.first_unstable, (count, ref.solid_count, r_bad, ref.first_unstable)
        if r_bad == -1:
            want = ref.f_next.astype(np.float64)
            assert np.array_equal(r_fn, want), "the single iterations' f_next is not the float32 reference's bit for bit: " + where(r_fn, want)
            for got, want in zip(r_macros, snapshot(ref)):
                assert np.array_equal(got, want.astype(np.float64)), "the single iterations' macros are not the float32 reference's snapshot"
            assert_forces_match(r_log, ref.forces, "single iterations")
    elif f2.reference_of(case).first_unstable == -1:
        ref = f2.reference_of(case)
        assert count == ref.solid_count and r_bad == -1, (count, ref.solid_count, r_bad)
        err, floor = oc.errors(r_fn, r_macros, ref), oc.floors_of_runs(f2.reference32_of(case), ref)
        record("f32_oracle_sweep2_contracted", case=case.k, model=case.model, periodic=case.periodic, steps=f2.steps_of(case), err_f=err[0],
               err_rho=err[1], err_u=err[2], floor_f=floor[0], floor_rho=floor[1], floor_u=floor[2])
        bad = oc.contracted_problems(err, floor)
        assert not bad, "the single iterations against the float64 reference: " + "; ".join(bad)
    with make(lbm, case) as ctx:
        assert ctx.initialise() == count
        for n in f2.issued_calls(case):
            ctx.step(n, case.of)
        assert_kernel(ctx, case, case.plan)
        assert ctx.first_unstable_step() == r_bad
        if r_bad != -1:
            return
        fn, macros, log = ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()
    cut = (interior(case, fn), interior(case, r_fn)) if f2.grouped(case) else (fn, r_fn)
    assert np.all(np.isfinite(r_fn)) and np.array_equal(*cut), "f_next is not the single iterations' bit for bit: " + where(fn, r_fn)
    for got, want in zip(macros, r_macros):
        assert np.array_equal(got, want), "macros differ"
    assert [r[0] for r in log] == [r[0] for r in r_log]
    for (t, fx, fy), (_, wx, wy) in zip(log, r_log):
        if not f2.grouped(case) or len(f2.bounds_of(case)) == 1:
            assert fx == wx and fy == wy, (t, fx, fy, wx, wy)
        else:       # (the strips' partial sums are added in another order)
            assert abs(fx - wx) <= 1e-5 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-5 * max(1.0, abs(wy)), (t, fx, fy, wx, wy)


@pytest.mark.parametrize("case", f2.fp32_cases(), ids=f2.case_id)
def test_fp32_case_equals_single_iterations(lbm, case):
    try:
        run_fp32_case(lbm, case)
    except AssertionError as e:
        raise AssertionError("%s\n%s" % (e, case)) from e


# ---- 3. the smallest periodic lattices on every strip plan ------------------------------------------------------------------------------
def expected_kernel(options, precision="f64"):
    """The family the plan pins, by its kernel's name: a silent fall-back to another family fails here."""
    deep = options.get("deep", 0)
    name = "k_stepc_col" if deep >= 6 else "k_stepd_tile" if deep else "k_step3_tile" if options.get("fuse") == 3 else \
        "k_step2_tile" if options.get("pair") else "k_step_site"
    return name + ("<float" if precision == "f32" else "<double")


def run_smallest(lbm, nx, ny, variant, options, precision="f64", roll=0):
    with lbm.Context(nx, ny, options=options, precision=precision, **f2.smallest_inputs(nx, ny, variant, roll)[0]) as ctx:
        count = ctx.initialise()
        assert ctx.periodic_y()
        for n, of in f2.SMALLEST_CALLS:
            ctx.step(n, of)
        assert ctx.first_unstable_step() == -1
        return count, ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.kernel_name().replace(" ", "")


@pytest.mark.parametrize("plan", list(PERIODIC_PLANS))
@pytest.mark.parametrize("nx,ny,variant", f2.SMALLEST_CASES, ids=lambda v: str(v))
def test_smallest_periodic_lattices_against_the_reference(lbm, nx, ny, variant, plan):
    """fp64, every strip plan: strict plans f_next bit for bit (the wrapped ghost rows included), contracted ones within 1e-10, the
    forces across the seam at the force bar; on the family the plan pins, or refused as the table beside the cases says."""
    if (nx, ny, plan) in f2.SMALLEST_REFUSED:
        with lbm.Context(nx, ny, options=PERIODIC_PLANS[plan], **f2.smallest_inputs(nx, ny, variant)[0]) as ctx:
            with pytest.raises(lbm.LbmError, match=f2.SMALLEST_REFUSED[nx, ny, plan]):
                ctx.initialise()
        return
    ref = f2.smallest_reference(nx, ny, variant)
    arith = f2.contracted(plan, 1)
    count, fn, macros, log, kernel = run_smallest(lbm, nx, ny, variant, PERIODIC_PLANS[plan])
    assert count == ref.solid_count
    assert kernel.startswith(expected_kernel(PERIODIC_PLANS[plan])), (plan, kernel)
    assert kernel.endswith(",%d>" % ((16 if variant != "plain" else 0) | arith)), (plan, kernel)
    if arith:
        rho, ux, uy = macros
        record("feature_sweep2_smallest", plan=plan, nx=nx, ny=ny, variant=variant,
               err_f=float(np.max(np.abs(fn - ref.f_next)) / np.max(np.abs(ref.f_next))), err_rho=float(np.max(np.abs(rho - ref.rho))),
               err_u=max(float(np.max(np.abs(ux - ref.ux))), float(np.max(np.abs(uy - ref.uy)))))
    assert_matches_reference(arith, fn, macros, log, ref, U_BAR_ABS)


# (the tall fp32 regions are BGK's alone: csrc/lbm_plan.hpp collision_models)
@pytest.mark.parametrize("nx,ny,variant,plan", [c + (p,) for c in f2.SMALLEST_CASES for p in f2.SMALLEST_F32_PLANS if c[2] == "plain" or p != "tall-f32"],
                         ids=lambda v: str(v))
def test_smallest_periodic_lattices_in_strict_fp32(lbm, nx, ny, variant, plan):
    """fp32 in strict arithmetic: f_next, the macro snapshot and the force rows against the float32 reference, bit for bit."""
    ref = f2.smallest_reference(nx, ny, variant, "f32")
    options = f2.plan_options(plan, 1)
    count, fn, macros, log, kernel = run_smallest(lbm, nx, ny, variant, options, "f32")
    assert count == ref.solid_count and ref.first_unstable == -1
    assert kernel.startswith(expected_kernel(options, "f32")) and kernel.endswith(",%d>" % (16 if variant != "plain" else 0)), (plan, kernel)
    if plan == "tall-f32":
        assert kernel.startswith("k_stepc_col<float,6,8,7,"), kernel
    want = ref.f_next.astype(np.float64)
    assert np.array_equal(fn, want), "f_next is not the float32 reference's bit for bit: " + where(fn, want)
    for got, want in zip(macros, snapshot(ref)):
        assert np.array_equal(got, want.astype(np.float64)), "the macros are not the float32 reference's snapshot"
    assert_forces_match(log, ref.forces, plan)


# ---- 4. roll invariance at the ragged heights -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rolled(lbm, nx, ny, plan, roll):
    return run_smallest(lbm, nx, ny, "plain", PERIODIC_PLANS[plan], roll=roll)


@pytest.mark.parametrize("plan", ["deep1", "deep7", "fast-fuse3"])
@pytest.mark.parametrize("nx,ny", [(65, 15), (130, 17)])
def test_roll_invariance_at_the_ragged_heights(lbm, nx, ny, plan):
    """Mask and profile rolled by 7 rows give the populations rolled by 7 rows, bit for bit: at heights that are no multiple of
    anything, no row is special (the tile edges, the edge bands and the wrap of the tables fall on other rows of the flow)."""
    _, a, _, la, _ = rolled(lbm, nx, ny, plan, 0)
    _, b, _, lb, _ = rolled(lbm, nx, ny, plan, 7)
    assert np.array_equal(np.roll(a[1:-1], 7, axis=0), b[1:-1]), where(np.roll(a[1:-1], 7, axis=0), b[1:-1])
    assert not force_problems(lb, la)
