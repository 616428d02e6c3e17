"""Every row of the table behind option "deep" (csrc/lbm_plan.hpp deep_shapes / region_kinds, as lbm_debug_deep_shapes prints it) on the
GPU, by the method of tests/test_gpu_col_parked.py: a pinned plan against the same context stepped ONE iteration per launch in the same
arithmetic mode, np.array_equal and never a tolerance.

130x70 with the default disc: every region height (24, 32, 40, 48) and both LDS tiles have a partial last column there at every depth and
a partial last band at all but one (64x24 at six iterations stores five whole bands of 14 rows; at five and seven it has one). Calls of 5, 6, 7, 8, 13 and 20 iterations under trailing_pair, each followed by one more iteration (a call that ended on a fused
launch leaves no snapshot of the previous iteration): on a whole domain they are single launches of 5, 6 and 7 iterations, 8 or 3 + 5,
6 + 7 or 7 + 6 and 20 = 7 + 7 + 6 (tests/test_deep_shapes_cpu.py holds the sequences), so every depth a shape's row offers is launched.
The launchers pick the kernel by walking that row, and kernel_name() must name the row's rows per thread, waves and depth."""
import functools

import numpy as np
import pytest

from tests.helpers import deep_shapes, lbm_gpu  # noqa: F401
from tests.test_deep_shapes_cpu import TABLE

pytestmark = pytest.mark.gpu

NX, NY = 130, 70
LENGTHS = (5, 6, 7, 8, 13, 20)
FORCE = (1e-5, 0.0)
ROWS = sorted((i, p, a) for i, row in TABLE.items() for p, a in row[2])      # (the literal the CPU test holds the library's table to)
# (row, nt, forced): BGK on every row, in both store policies where the row's kind has instantiations of both; the forced model on the
# two kinds of object it has beside BGK's (64x32 regions: id 7; 64x40 regions: id 11)
CASES = [(r, nt, False) for r in ROWS for nt in ((1, 0) if any(p == "nt+plain" for _, p, _ in TABLE[r[0]][3]) else (1,))] + \
        [(r, 1, True) for r in ROWS if r[0] in (7, 11)]


def series(lbm, precision, options, forced):
    """(kernel name, [(f_current, f_next, macros) after each call of LENGTHS and the single iteration behind it])"""
    with lbm.Context(NX, NY, precision=precision, inlet_velocity=0.05, options=dict(options, trailing_pair=1)) as ctx:
        if forced:
            ctx.set_forcing(*FORCE)
        assert ctx.initialise() > 0             # (the disc)
        states = []
        for n in LENGTHS:
            ctx.step(n, 0)
            ctx.step(1, 0)
            states.append((ctx.populations("f_current"), ctx.populations("f_next"), ctx.macros()))
        assert ctx.first_unstable_step() == -1
        return ctx.kernel_name(), states


@functools.lru_cache(maxsize=None)
def one_iteration_series(lbm, precision, arith, forced):
    name, states = series(lbm, precision, dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=arith), forced)
    assert name.startswith("k_step_site<"), name
    return states


@pytest.mark.parametrize("row,nt,forced", CASES, ids=["deep%d-%s-%s-nt%d%s" % (r + (nt, "-forced" if f else "")) for r, nt, f in CASES])
def test_every_row_equals_single_iterations(lbm, row, nt, forced):
    deep, precision, arith = row
    r = deep_shapes()[row]
    name, got = series(lbm, precision, dict(tune=0, layout=1, pair_ty=12, xcd=1, nt=nt, alternate=0, deep=deep, arith=arith), forced)
    t, ar = "double" if precision == "f64" else "float", arith + (8 if forced else 0)
    if r.family == "registers":
        nts = "true" if nt and dict((d, p) for d, p, _ in r.offered)[r.depth] == "nt+plain" else "false"
        assert name == "k_stepc_col<%s,%d,%d,%d,%s,%d>" % (t, r.rows, r.waves, r.depth, nts, ar), name
        # a partial last column at every depth launched and a partial last band at one at least (five bands of 14 rows: 64x24 at six iterations)
        assert r.h == r.rows * r.waves and all(NX % (r.w - 2 * (d - 1)) for d, _, _ in r.offered) and any(NY % (r.h - 2 * (d - 1)) for d, _, _ in r.offered)
    else:
        assert name == "k_stepd_tile<%s,%d,%d,%d,%d>" % (t, r.w, r.h, r.depth, ar), name
        assert NY % r.h and NX % r.w
    want = one_iteration_series(lbm, precision, arith, forced)
    for n, g, w in zip(LENGTHS, got, want):
        assert np.array_equal(g[1], w[1]), (row, n, "f_next")
        assert np.array_equal(g[0], w[0]), (row, n, "f_current")
        for a, b in zip(g[2], w[2]):
            assert np.array_equal(a, b), (row, n, "macros")


def test_a_model_without_the_kind_is_refused(lbm):
    """collision_models grants the 64x48 regions to BGK alone: the setter of the option and the setter of the model both say so."""
    with lbm.Context(NX, NY, precision="f32", smagorinsky=0.17) as ctx:
        with pytest.raises(lbm.LbmError, match=r"deep 8 \(64x48 regions in registers\) has no Smagorinsky \(LES\) kernel"):
            ctx.set_option("deep", 8)
    with lbm.Context(NX, NY, precision="f32", options=dict(tune=0, deep=8)) as ctx:
        with pytest.raises(lbm.LbmError, match=r"deep 8 \(64x48 regions in registers\) has no two-relaxation-time \(TRT\) kernel"):
            ctx.set_trt(0.25)
