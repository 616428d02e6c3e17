"""Mixed blocks of the register kernel (csrc/lbm_kernel_col.hpp "Mixed blocks"): in a tile that is not lean as a whole — a wall tile, a
partial band, a strip's edge — every wave whose rows are plain interior fluid at every level (csrc/lbm_kernels.hpp wave_plain) runs the
lean path, the other waves of the same block the general path, with one barrier per level between them.

DESIGN.md §3: every formulation performs the same per-cell operation sequence within an arithmetic mode, so every comparison below is
np.array_equal on the populations and equality of first_unstable_step against the same context stepped at ONE iteration per launch
(k_step_site), never a tolerance.

The grids are the smallest that still have middle tile columns (the x-conditions of the lean path) and wall tiles of several waves:
  170 x 57..62   three or four tile columns, two to four bands: the top wall row lands on six consecutive region rows, hence on every
                 row index of a wave and in two or three wave indices, in a partial top band of every height; the bottom wall row stands
                 on region row D - 1 (its place in a wave moves with the depth and the rows per thread)
  230 x 90       the settings that must switch the verdict off for the waves they reach: free-slip and moving walls, periodic y, pressure
                 and velocity ports, an inlet profile, one solid cell next to either wall inside a middle tile, a group of two strips
Shapes: every `deep` of the register family: 64x32 regions at six and seven iterations (fp64 contracted and fp32: 8 waves x 4 rows; fp64
strict: 12 x 2), 64x40 at six and seven (fp64 contracted, the parked form), fp32 64x48 (contracted 12 x 4, strict 8 x 6).
Variants: non-temporal and plain stores, non-temporal level-1 loads, both walk directions (alternate), split 0 and 3."""
import functools

import numpy as np
import pytest

from tests.helpers import every_row_differs, lbm_gpu  # noqa: F401
from tests.ports_reference import PRESSURE, VELOCITY
from tests.reference import FREESLIP, moving

pytestmark = pytest.mark.gpu

PIN = dict(tune=0, layout=1, pair_ty=12, xcd=1)
ONE = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)             # one iteration per launch
# (precision, arith, deep): 64x32 at six / seven iterations, 64x40 at six / seven, fp32 64x48, strict fp64 12 x 2
SHAPES = [("f64", 1, 7), ("f64", 1, 9), ("f64", 1, 10), ("f64", 1, 11), ("f32", 1, 8), ("f32", 0, 8), ("f64", 0, 7)]
WHOLE_ONLY = (10, 11)                                               # the 64x40 regions run on whole walled domains only
VARIANTS = [dict(nt=1, ntl=0, alternate=0, split=0), dict(nt=0, ntl=1, alternate=1, split=0), dict(nt=1, ntl=1, alternate=1, split=3, split_min=1)]
CALLS = ((29, 0), (13, 6))                                          # several deep launches in both walk directions, a remainder, two force outputs (iterations 30 and 36)
KW = dict(tau=0.6, inlet_velocity=0.05)


def shape_id(s):
    return "%s-%s-deep%d" % (s[0], "contracted" if s[1] else "strict", s[2])


def run(lbm, nx, ny, opts, precision, plant=None, **kw):
    with lbm.Context(nx, ny, precision=precision, options=opts, **dict(KW, **kw)) as c:
        c.initialise()
        if plant is not None:
            c.step(plant[0], 0)
            f = c.populations("f_current")
            f[plant[2] + 1, plant[1] + 1, 0] = 1e9            # (the rest population: it stays in its cell; far above 1e5 after the collision too)
            c.set_f_current(f)
        for steps, of in CALLS:
            c.step(steps, of)
        return dict(f_current=c.populations("f_current"), f_next=c.populations("f_next"), unstable=c.first_unstable_step(),
                    log=c.drain_force_log(), kernel=c.kernel_name())


@functools.lru_cache(maxsize=None)
def one_iteration(lbm, nx, ny, precision, arith, setting, plant=None):
    r = run(lbm, nx, ny, dict(ONE, arith=arith), precision, plant=plant, **SETTINGS[setting](nx, ny))
    assert "k_stepc_col" not in r["kernel"]
    for k in ("f_current", "f_next"):
        r[k].setflags(write=False)
    return r


def assert_same(got, ref, what, nan=False):
    assert "k_stepc_col" in got["kernel"], (what, got["kernel"])
    assert got["unstable"] == ref["unstable"], (what, got["unstable"], ref["unstable"])
    for k in ("f_current", "f_next"):
        assert np.array_equal(got[k], ref[k], equal_nan=nan), (what, k, "first differing cell (row, column) %s" %
                                                             (np.argwhere(np.any(got[k] != ref[k], axis=-1))[:1] - 1).tolist())
    if not nan:
        assert got["log"] == ref["log"] and len(ref["log"]) == 2, what


def one_cell_masks(nx, ny):
    m = np.zeros((ny, nx), np.uint8)
    m[1, 120] = m[ny - 2, 70] = 1          # next to the bottom wall and next to the top wall, each inside a middle tile column
    return m


SETTINGS = {
    "plain": lambda nx, ny: {},
    "walls": lambda nx, ny: dict(walls=(FREESLIP, moving(0.04))),
    "walls-swapped": lambda nx, ny: dict(walls=(moving(-0.03), FREESLIP)),
    "periodic": lambda nx, ny: dict(periodic_y=True),
    "ports": lambda nx, ny: dict(ports=((PRESSURE, 1.015), (VELOCITY, 0.03))),
    "profile": lambda nx, ny: dict(inlet_profile=every_row_differs(ny, 0.05)),
    "one-cell-mask": lambda nx, ny: dict(solid=one_cell_masks(nx, ny)),
}


@pytest.mark.parametrize("ny", [57, 58, 59, 60, 61, 62])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_wall_rows_on_every_row_of_a_wave(lbm, shape, ny):
    precision, arith, deep = shape
    ref = one_iteration(lbm, 170, ny, precision, arith, "plain")
    assert ref["unstable"] == -1
    for v in VARIANTS:
        got = run(lbm, 170, ny, dict(PIN, deep=deep, arith=arith, **v), precision)
        assert_same(got, ref, (shape, ny, v))


# (periodic y: the 64x40 regions run on whole walled domains only, lbm_initialise refuses the pair)
@pytest.mark.parametrize("shape,setting", [(sh, st) for st in SETTINGS if st != "plain" for sh in SHAPES if not (st == "periodic" and sh[2] in WHOLE_ONLY)],
                         ids=lambda v: shape_id(v) if isinstance(v, tuple) else v)
def test_settings_that_reach_a_wave(lbm, shape, setting):
    precision, arith, deep = shape
    nx, ny = 230, 90
    ref = one_iteration(lbm, nx, ny, precision, arith, setting)
    assert ref["unstable"] == -1
    for v in (VARIANTS[:2] if setting == "periodic" else VARIANTS[::2]):         # (row-range launches exist for a whole walled domain only)
        got = run(lbm, nx, ny, dict(PIN, deep=deep, arith=arith, **v), precision, **SETTINGS[setting](nx, ny))
        assert_same(got, ref, (shape, setting, v))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] not in WHOLE_ONLY], ids=shape_id)
def test_two_strips(lbm, shape):
    """Edge tiles at y_start != 0 and partial bands that are no domain's top: the faces of two strips of 45 rows."""
    precision, arith, deep = shape
    nx, ny = 230, 90
    ref = one_iteration(lbm, nx, ny, precision, arith, "profile")
    opts = dict(PIN, nt=1, alternate=0, deep=deep, arith=arith)
    with lbm.Group(nx, ny, 2, options=opts, precision=precision, inlet_profile=every_row_differs(ny, 0.05), **KW) as g:
        g.initialise()
        for steps, of in CALLS:
            g.step(steps, of)
        assert g.first_unstable_step() == ref["unstable"] == -1
        assert np.array_equal(g.populations("f_next"), ref["f_next"])
        assert np.array_equal(g.populations("f_current")[1:-1, 1:-1], ref["f_current"][1:-1, 1:-1])      # (interior: the ghost frame is the gather's)
        log = g.drain_force_log()                        # (the strips' sums are added in another order: the strips-against-whole bar)
        assert [r[0] for r in log] == [r[0] for r in ref["log"]] and len(log) == 2
        for (_, fx, fy), (_, wx, wy) in zip(log, ref["log"]):
            assert abs(fx - wx) <= 1e-13 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-13 * max(1.0, abs(wy))


# (x, y) of the planted value on 230 x 90 at seven iterations on 64x40 regions (52 x 28 outputs; tile column 2 holds x 104..155 and reads
# 98..161; the bottom tile row reads rows -6..33, wall row 0 in wave 1, waves 2..7 plain; the top one outputs 84..89 and reads 78..117, wall
# row 89 in wave 2, waves 0 and 1 plain) and the matching places of the other shapes, which differ by a row or two
PLANTS = {
    "plain-wave-bottom-tile": (120, 6), "plain-wave-top-tile": (120, 85), "ring-left-of-outputs": (100, 7), "ring-right-of-outputs": (158, 86),
    "ring-above-bottom-tile": (121, 30), "ring-below-top-tile": (119, 80), "general-wave-bottom": (120, 2), "bottom-wall-row": (122, 0),
    "general-wave-top": (120, 88), "top-wall-row": (118, 89),
}


@pytest.mark.parametrize("where", list(PLANTS))
@pytest.mark.parametrize("shape", [("f64", 1, 11), ("f64", 1, 7), ("f64", 0, 7), ("f32", 1, 8)], ids=shape_id)
def test_planted_value_is_counted_alike(lbm, shape, where):
    """One value above 1e5 planted after a few iterations, in a plain wave of a wall tile, in its halo rings and in the general wave beside
    it: both paths must name the same first unstable iteration and leave the same populations. What this can and cannot tell: the planted
    value is counted by level 1 of the first deep launch, in its own tile and in every tile whose rings hold it, and the word is a
    minimum, so this holds the level-1 counts (every lane on the lean path, the lanes with a column of loaded rows on the general path)
    against each other; the counts of levels 2..D (lane_ok against lane_ok && col_in && y <= y_end + HW - L) cannot move that minimum
    here. Their agreement for a plain wave is held cell by cell and level by level by tests/test_boundary_waves_cpu.py, and the
    golden unstable cases of tests/test_gpu_boundary_tiles.py, which blow up on their own at a later level, run mixed blocks too."""
    precision, arith, deep = shape
    nx, ny = 230, 90
    plant = (11,) + PLANTS[where]
    ref = one_iteration(lbm, nx, ny, precision, arith, "plain", plant)
    assert 0 <= ref["unstable"] <= 11, ref["unstable"]
    for v in VARIANTS[::2]:
        got = run(lbm, nx, ny, dict(PIN, deep=deep, arith=arith, **v), precision, plant=plant)
        assert_same(got, ref, (shape, where, v), nan=True)
