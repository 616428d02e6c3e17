"""The register kernel's boundary tiles (csrc/lbm_kernel_col.hpp, the general path): tiles whose halo rings touch a wall, the inlet or
outlet column, a partial band or column, a solid cell, or a strip's edge.

That path issues the loads of all its rows before the first update, gives a cell outside the domain its ghost value once (level 1) and
skips it at every later level, and fetches a row's inlet velocity and a thread's mask words once per launch. DESIGN.md §3: every
formulation performs the same per-cell operation sequence within an arithmetic mode, so every comparison below is np.array_equal
against the same context stepped at ONE iteration per launch (k_step_site), never a tolerance.

The shapes are the smallest at which that code can go wrong (output tiles at five / six / seven iterations per launch: 56x24, 54x22,
52x20 from 64x32 regions; the strict fp64 shape has 64x24 regions):
  130x50   three by three tiles at six iterations: one lean centre tile, eight general ones, a partial last column and a partial last band
  70x20    fewer rows than a region is high: every block has rows outside the domain below and above (rows skipped at every level; the
           first and the last wave read their own exchange slot)
  200x90   an inlet profile with a different value on every row, a schedule table, a moving top wall and a free-slip bottom wall: each of
           a thread's rows needs its own inlet velocity at every level
  200x90   the same lattice with solid cells in all rows of a thread, at the tile corners, in column 0 and in row 0 next to the wall
  256x400  as a group of two strips of 200 rows: edge tiles at y_start != 0
  the two golden unstable cases at 32 and at 320 rows: the first unstable iteration"""
import functools

import numpy as np
import pytest

from tests.helpers import (CtxRun, assert_group_is_whole, assert_same_results, every_row_differs, golden_params, lbm_gpu, load_golden,  # noqa: F401
                           masks)
from tests.reference import FREESLIP, moving

pytestmark = pytest.mark.gpu

PIN = dict(tune=0, layout=1, pair_ty=12, xcd=1)
ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)             # one iteration per launch
DEEPS = {"f64": (7, 6, 9), "f32": (7, 6, 9, 8)}                     # six, five, seven iterations per launch; fp32 also the tall regions
SPLITS = (0, 3)
CALLS = ((61, 0), (37, 10))


def corners_and_edges(nx, ny):
    """Solid cells in all four rows of one thread (a block twelve rows high standing on the bottom wall, so in row 0 too), at the tile
    corners of every depth, in column 0 and in the last column, and single cells (one in row 0, one in the top row)."""
    m = masks(nx, ny)
    out = m["bottom-block"] | m["inlet-outlet"] | m["single-cells"]
    for ow, oh in ((56, 24), (54, 22), (52, 20)):
        out[oh - 1:oh + 1, ow - 1:ow + 1] = 1
        out[2 * oh - 1:2 * oh + 1, 3 * ow - 1] = 1
    return out


def case_kw(name):
    """(nx, ny, Context keywords) of a case."""
    if name == "130x50":
        return 130, 50, dict(inlet_velocity=0.05)
    if name == "70x20":
        return 70, 20, dict(inlet_velocity=0.05)
    nx, ny = 200, 90
    kw = dict(inlet_velocity=0.05, inlet_profile=every_row_differs(ny, 0.05), inlet_schedule=(np.linspace(0.25, 1.0, 16), "hold"),
              walls=(FREESLIP, moving(0.04)))
    if name == "200x90-mask":
        kw["solid"] = corners_and_edges(nx, ny)
    return nx, ny, kw


def run_calls(lbm, nx, ny, opts, precision, **kw):
    with lbm.Context(nx, ny, precision=precision, options=opts, **kw) as ctx:
        n = ctx.initialise()
        for steps, of in CALLS:
            ctx.step(steps, of)
        return CtxRun(n, ctx.populations("f_current"), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(),
                      ctx.first_unstable_step(), ctx.kernel_name(), ctx.plan())


@functools.lru_cache(maxsize=None)
def one_iteration_run(lbm, name, precision, arith):
    nx, ny, kw = case_kw(name)
    return run_calls(lbm, nx, ny, dict(ONE, arith=arith), precision, **kw)


@pytest.mark.parametrize("arith", [0, 1], ids=["strict", "contracted"])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", ["130x50", "70x20", "200x90-inlet-walls", "200x90-mask"])
def test_deep_launches_equal_single_iterations(lbm, name, precision, arith):
    nx, ny, kw = case_kw(name)
    ref = one_iteration_run(lbm, name, precision, arith)
    assert "k_stepc_col" not in ref.kernel_name and len(ref.force_log) == 3
    if name == "200x90-mask":
        assert ref.solid_count == int(kw["solid"].sum())
    for deep in DEEPS[precision]:
        for split in SPLITS:
            opts = dict(PIN, nt=1, alternate=int(split == 0), deep=deep, arith=arith, split=split, split_min=1)
            got = run_calls(lbm, nx, ny, opts, precision, **kw)
            assert "k_stepc_col" in got.kernel_name, (deep, split, got.kernel_name)
            try:
                assert_same_results(got, ref, rows=3)
            except AssertionError as e:
                raise AssertionError("deep %d split %d (%s): %s" % (deep, split, got.kernel_name, e)) from e


@pytest.mark.parametrize("rows", [32, 320])
@pytest.mark.parametrize("name", ["g8a_unstable_128x32", "g8b_unstable_128x32"])
def test_first_unstable_iteration(lbm, name, rows):
    g = load_golden(name)
    kw = dict(golden_params(g), ny=rows)
    steps, of = int(g["p_steps"]), int(g["p_output_frequency"])

    def first_unstable(opts):
        with lbm.Context(options=opts, **kw) as c:
            c.initialise()
            c.step(steps, of)
            return c.first_unstable_step()
    for arith in (0, 1):
        want = first_unstable(dict(ONE, arith=arith))
        print(f"{name} at {rows} rows, arith {arith}: first unstable iteration {want}")
        if rows == 32 and arith == 0:
            assert want == int(g["unstable_t"])
        got = {(deep, split): first_unstable(dict(PIN, nt=1, alternate=0, deep=deep, arith=arith, split=split, split_min=1))
               for deep in DEEPS["f64"] for split in SPLITS}
        assert got == dict.fromkeys(got, want), (arith, want, got)


@pytest.mark.parametrize("arith", [0, 1], ids=["strict", "contracted"])
def test_two_strips_of_200_rows_are_the_whole(lbm, arith):
    nx, ny, steps, of = 256, 400, 61, 20
    kw = dict(inlet_velocity=0.05, inlet_profile=every_row_differs(ny, 0.05))
    opts = dict(PIN, nt=1, alternate=0, deep=7, arith=arith)
    with lbm.Context(nx, ny, options=opts, **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        assert "k_stepc_col" in whole.kernel_name() and whole.first_unstable_step() == -1
        w = (whole.macros(), whole.populations("f_next"), whole.drain_force_log())
    assert len(w[2]) == 4
    with lbm.Group(nx, ny, 2, options=opts, **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)
