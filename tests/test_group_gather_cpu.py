"""The rules by which the library puts the results of the row strips of a group together (csrc/lbm_gather.hpp, used by every
lbm_group_get_* / lbm_group_drain_* call), through lbm_debug_gather: no device. Planes are stacked at row y_start (frames: y_start / k),
ghost-inclusive populations take the physical ghost rows from the end strips only, and a sum is strip 0's value followed by
left-to-right additions. Held against np.concatenate and a Python loop."""
import importlib

import numpy as np
import pytest

from tests.helpers import PKG

NX, ROWS = 8, (12, 16, 20)
NY = sum(ROWS)
BOUNDS = [(sum(ROWS[:i]), r) for i, r in enumerate(ROWS)]


@pytest.fixture(scope="module")
def gather():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    return pkg.debug_gather


def strips(rng, planes, dtype, k=1):
    return [rng.standard_normal((planes, r // k, NX // k)).astype(dtype) for r in ROWS]


def test_six_double_planes_are_stacked_by_y_start_and_cut_out_again(gather):
    parts = strips(np.random.default_rng(1), 6, np.float64)
    whole = np.full((6, NY, NX), np.nan)
    gather("stack", BOUNDS, NX, NY, parts, whole, planes=6)
    assert np.array_equal(whole, np.concatenate(parts, axis=1))
    back = [np.full_like(p, np.nan) for p in parts]
    gather("unstack", BOUNDS, NX, NY, back, whole, planes=6)
    assert all(np.array_equal(b, p) for b, p in zip(back, parts))


def test_four_float_planes_of_a_frame_are_stacked_at_y_start_over_k(gather):
    k = 4
    parts = strips(np.random.default_rng(2), 4, np.float32, k)
    assert [p.shape[1] for p in parts] == [3, 4, 5]
    whole = np.full((4, NY // k, NX // k), np.nan, dtype=np.float32)
    gather("stack_f32", BOUNDS, NX, NY, parts, whole, k=k, planes=4)
    assert np.array_equal(whole, np.concatenate(parts, axis=1))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_populations_take_the_physical_ghost_rows_from_the_end_strips(gather, n):
    rows = ROWS[:n]
    ny = sum(rows)
    bounds = [(sum(rows[:i]), r) for i, r in enumerate(rows)]
    rng = np.random.default_rng(3)
    parts = [rng.standard_normal((r + 2, NX + 2, 9)) for r in rows]
    whole = np.full((ny + 2, NX + 2, 9), np.nan)
    gather("populations", bounds, NX, ny, parts, whole)
    want = np.concatenate([parts[0][:1]] + [p[1:-1] for p in parts] + [parts[-1][-1:]], axis=0)
    assert np.array_equal(whole, want)


def test_a_sum_is_strip_0_then_left_to_right_additions(gather):
    rng = np.random.default_rng(4)
    parts = [rng.standard_normal(NX) * 10.0 ** rng.integers(-8, 8, NX) for _ in ROWS]
    parts[0][0], parts[1][0], parts[2][0] = 1e16, 1.0, -1e16          # the order shows: (1e16 + 1) - 1e16 == 0, not 1
    total = np.full(NX, np.nan)
    gather("sum", BOUNDS, NX, NY, parts, total)
    want = parts[0].copy()
    for p in parts[1:]:
        want = want + p
    assert np.array_equal(total, want) and total[0] == 0.0


def test_a_lone_negative_zero_stays_negative(gather):
    total = np.full(2, np.nan)
    gather("sum", BOUNDS[:1], 2, NY, [np.array([-0.0, 0.0])], total)
    assert np.signbit(total).tolist() == [True, False]
    gather("sum", BOUNDS, 2, NY, [np.array([-0.0, -0.0]), np.array([-0.0, 0.0]), np.array([-0.0, -0.0])], total)
    assert np.signbit(total).tolist() == [True, False]                 # IEEE: -0 + -0 = -0, -0 + +0 = +0


def test_the_hook_refuses_strips_outside_the_lattice(gather):
    pkg = importlib.import_module(PKG)
    with pytest.raises(pkg.LbmError, match="outside"):
        gather("stack", [(0, 12), (12, NY)], NX, NY, [np.zeros((1, 12, NX)), np.zeros((1, NY, NX))], np.zeros((1, NY, NX)))
