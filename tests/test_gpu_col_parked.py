"""The register kernel on 64x40 fp64 regions with every thread's top row parked in LDS (csrc/lbm_kernel_col.hpp "Parked top row";
plans `deep` 10 / 11: six / seven iterations per launch, contracted arithmetic, whole domains).

DESIGN.md §3: every formulation performs the same per-cell operation sequence within an arithmetic mode, so every comparison below is
np.array_equal — contracted against contracted — with the same context stepped at ONE iteration per launch (k_step_site), never a
tolerance. Every pinned run must name the five-row kernel, so nothing here can pass on another kernel.

The shapes are the smallest with every tile class. Output tiles are 54x30 (six iterations, regions start five rows below their band)
and 52x28 (seven, six rows below); a thread's parked row is region row 4 mod 5.
  130x70   three tile columns, bands of 30 + 30 + 10: lean and general tiles, a partial last column and band. The north wall (row 69) is
           region row 14 of the last band at six iterations and 19 at seven: a parked row
  130x69   the first ghost row above the north wall is that parked row instead: skipped at levels 2..D, its north-going three must
           stand in both exchange buffers
  118x64   another partial band (30 + 30 + 4) and column
  the south wall needs no shape of its own: row -1 (six iterations) / row -2 (seven) is region row 4 of every bottom band; the
  alternate walk issues those bands last
  270x120  the default disc (centre 54, 60, radius 6) across the tile seams x = 54 and y = 60"""
import functools

import numpy as np
import pytest

from tests.helpers import CtxRun, every_row_differs, lbm_gpu  # noqa: F401
from tests.reference import FREESLIP, moving

pytestmark = pytest.mark.gpu

ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=1)        # one iteration per launch
PIN = dict(tune=0, layout=1, pair_ty=12, xcd=1, arith=1)
IDS = (10, 11)
WALKS = (dict(nt=1, ntl=0, alternate=0, split=0), dict(nt=0, ntl=1, alternate=1, split=3, split_min=1))
CALLS = ((20, 0), (13, 5))
KERNEL = "k_stepc_col<double,5,8,"


def single_cells(nx, ny):
    """One-cell obstacles on fifteen consecutive rows (every row of a thread, in several bands, at both depths), and at lanes 0 / 1 and
    62 / 63 of the second tile column's regions: x = 49, 50, 111, 112 at six iterations, 46, 47, 108, 109 at seven."""
    m = np.zeros((ny, nx), np.uint8)
    for k in range(15):
        m[20 + k, 30 + 4 * k] = 1
    for x in (49, 111, 46, 108):
        m[24, x] = m[53, x + 1] = 1            # rows 4 mod 5 and 3 mod 5
        m[40, x] = 1                           # row 0 mod 5
    return m


def case_kw(name):
    if name == "270x120-disc":
        return 270, 120, dict(inlet_velocity=0.05)
    if name == "130x70-cells":
        return 130, 70, dict(inlet_velocity=0.05, solid=single_cells(130, 70))
    if name == "130x70-inlet-walls":
        return 130, 70, dict(inlet_velocity=0.05, inlet_profile=every_row_differs(70, 0.05),
                             inlet_schedule=(np.linspace(0.25, 1.0, 16), "hold"), walls=(FREESLIP, moving(0.04)))
    if name == "130x70-walls-swapped":
        return 130, 70, dict(inlet_velocity=0.05, walls=(moving(-0.03), FREESLIP))
    nx, ny = (int(v) for v in name.split("x"))
    return nx, ny, dict(inlet_velocity=0.05)


def run_calls(lbm, name, opts, calls=CALLS, **more):
    nx, ny, kw = case_kw(name)
    with lbm.Context(nx, ny, options=opts, **dict(kw, **more)) as ctx:
        n = ctx.initialise()
        for steps, of in calls:
            ctx.step(steps, of)
        return CtxRun(n, ctx.populations("f_current"), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(),
                      ctx.first_unstable_step(), ctx.kernel_name(), ctx.plan())


@functools.lru_cache(maxsize=None)
def one_iteration_run(lbm, name, calls=CALLS, trailing_pair=0, model=()):
    return run_calls(lbm, name, dict(ONE, trailing_pair=trailing_pair), calls, **dict(model))


def assert_equal_runs(got, ref, what):
    assert got.kernel_name.startswith(KERNEL), (what, got.kernel_name)
    assert "k_stepc_col" not in ref.kernel_name
    assert got.solid_count == ref.solid_count and got.first_unstable == ref.first_unstable == -1, what
    assert np.array_equal(got.f_next, ref.f_next), what
    assert np.array_equal(got.f_current, ref.f_current), what
    for x, y in zip(got.macros, ref.macros):
        assert np.array_equal(x, y), what
    assert got.force_log == ref.force_log, what


@pytest.mark.parametrize("name", ["130x70", "130x69", "118x64", "270x120-disc", "130x70-cells", "130x70-inlet-walls", "130x70-walls-swapped"])
def test_pinned_plans_equal_single_iterations(lbm, name):
    ref = one_iteration_run(lbm, name)
    assert len(ref.force_log) == 3                  # iterations 20, 25, 30
    if name == "130x70-cells":
        assert ref.solid_count == int(single_cells(130, 70).sum())
    for deep in IDS:
        for walk in WALKS:
            got = run_calls(lbm, name, dict(PIN, deep=deep, **walk))
            assert got.kernel_name.startswith(KERNEL + "%d," % (6 if deep == 10 else 7)), got.kernel_name
            assert_equal_runs(got, ref, (name, deep, walk))


@pytest.mark.parametrize("trailing_pair", [0, 1])
@pytest.mark.parametrize("steps", [5, 6, 7, 13, 20])
def test_call_lengths_run_every_depth(lbm, steps, trailing_pair):
    """5, 6 and 7 are single launches of the remainder depths (with trailing_pair; without it the call ends on one iteration), 13 = 7 + 6
    or 6 + 7, 20 = 7 + 7 + 6: both ids meet all three kernels. A call that ended on a fused launch leaves no snapshot of the previous
    iteration, so one more iteration follows it before the accessors are read."""
    calls = ((steps, 0), (1, 0)) if trailing_pair else ((steps, 0),)
    ref = one_iteration_run(lbm, "130x70", calls, trailing_pair)
    for deep in IDS:
        got = run_calls(lbm, "130x70", dict(PIN, deep=deep, nt=1, ntl=0, alternate=0, trailing_pair=trailing_pair), calls)
        assert_equal_runs(got, ref, (steps, trailing_pair, deep))


@pytest.mark.parametrize("model,arith", [((("trt_magic", 0.25),), 5), ((("smagorinsky", 0.17),), 3)], ids=["trt", "les"])
def test_other_collision_models_have_the_shape(lbm, model, arith):
    """Their kernels keep four waves per SIMD without scratch on this shape (lbm_plan.hpp collision_models) and are built."""
    ref = one_iteration_run(lbm, "130x70", CALLS, 0, model)
    for deep in IDS:
        got = run_calls(lbm, "130x70", dict(PIN, deep=deep, nt=0, ntl=1, alternate=1), **dict(model))
        assert got.kernel_name.endswith(",%d>" % arith), got.kernel_name
        assert_equal_runs(got, ref, (model, deep))


def test_the_shape_is_refused_where_it_does_not_exist(lbm):
    with lbm.Context(130, 70, precision="f32") as ctx:
        with pytest.raises(lbm.LbmError, match="fp64 only"):
            ctx.set_option("deep", 10)
    with lbm.Context(130, 70, options=dict(tune=0, deep=11, arith=0)) as ctx:
        with pytest.raises(lbm.LbmError, match="contracted arithmetic on whole domains only"):
            ctx.initialise()
    with lbm.Context(130, 70, y_start=0, local_ny=35, options=dict(tune=0, deep=10, arith=1)) as ctx:
        with pytest.raises(lbm.LbmError, match="contracted arithmetic on whole domains only"):
            ctx.initialise()


def test_first_unstable_iteration(lbm):
    """tau 0.505, U 0.1 on 400x100 diverges: the deep launches report the iteration the single-iteration run reports (76)."""
    def first_unstable(opts):
        with lbm.Context(400, 100, tau=0.505, inlet_velocity=0.1, options=opts) as c:
            c.initialise()
            c.step(120, 0)
            return c.first_unstable_step(), c.kernel_name()
    want, _ = first_unstable(ONE)
    print("first unstable iteration of the single-iteration run:", want)
    assert want == 76
    for deep in IDS:
        for walk in WALKS:
            got, kernel = first_unstable(dict(PIN, deep=deep, **walk))
            assert kernel.startswith(KERNEL) and got == want, (deep, walk, got, kernel)
