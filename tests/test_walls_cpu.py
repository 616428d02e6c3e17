"""The walls of lbm_set_wall without a GPU: the kernels' wall rule (lbm_debug_wall_rule: the very inline function, compiled for the
host) against the table of include/lbm_hip.h, and the argument errors that need no device (the library's and lbm_solver's). (The
reference loop with two no-slip walls is pinned to the unmodified oracle in tests/test_reference_cpu.py.)"""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.helpers import lbm_cpu, solver  # noqa: F401
from tests.reference import FREESLIP, NOSLIP, moving, wall_kind_k, wall_rule


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("wall", [NOSLIP, FREESLIP, moving(0.08), moving(-0.03), moving(1.0 / 3.0)])
@pytest.mark.parametrize("side", [0, 1])
def test_wall_rule_hook_against_the_table(lbm, side, wall, precision):
    """Every side x kind on random cells. The table is evaluated in the element type: the inputs and k are rounded to it first, and each
    corrected population is one IEEE addition in it."""
    T = np.float64 if precision == "f64" else np.float32
    kind, k = wall_kind_k(wall)
    rng = np.random.default_rng(17 + side)
    cells = rng.random((64, 9)) * 0.5
    cells[0] = -0.0                                     # kinds 0 and 1 only move values: the sign of a zero survives
    u_w = wall[1] if kind == 2 else 0.0
    for f in cells:
        got = lbm.debug_wall_rule(("south", "north")[side], kind, u_w, f, precision)
        want = wall_rule(f.astype(T), side, kind, T(k)).astype(np.float64)
        assert want.dtype == np.float64 and np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        # the pair sums — mass — are those of bounce-back, to the rounding of the one addition
        noslip = wall_rule(f.astype(T), side, 0, T(0)).astype(np.float64)
        pair = (5, 6) if side == 0 else (7, 8)
        assert abs((got[pair[0]] + got[pair[1]]) - (noslip[pair[0]] + noslip[pair[1]])) <= 4 * np.finfo(T).eps
        if kind == 2:
            assert not np.array_equal(got, noslip)


def test_wall_argument_errors_without_a_device(lbm):
    L = lbm.lib()
    f = (C.c_double * 9)(*([0.1] * 9))
    out = (C.c_double * 9)()
    k, u = C.c_int(), C.c_double()
    assert L.lbm_set_wall(None, 0, 1, 0.0) == -1 and b"null context" in L.lbm_last_error()
    assert L.lbm_get_wall(None, 0, C.byref(k), C.byref(u)) == -1 and b"null context" in L.lbm_last_error()
    # the checks lbm_set_wall shares with the hook (the GPU file runs them on a context)
    for args, text in (((2, 0, 0.0), b"side"), ((-1, 0, 0.0), b"side"), ((0, 3, 0.0), b"kind"), ((0, -1, 0.0), b"kind"),
                       ((0, 2, float("nan")), b"velocity"), ((1, 2, float("inf")), b"velocity"), ((1, 2, 1.0), b"velocity"),
                       ((0, 2, -1.5), b"velocity"), ((0, 0, 0.01), b"no-slip"), ((1, 1, -0.01), b"free-slip")):
        assert L.lbm_debug_wall_rule(args[0], args[1], args[2], 0, f, out) == -1, args
        assert text in L.lbm_last_error(), (args, L.lbm_last_error())
    assert L.lbm_debug_wall_rule(0, 1, 0.0, 2, f, out) == -1 and b"precision" in L.lbm_last_error()
    assert L.lbm_debug_wall_rule(0, 1, 0.0, 0, None, out) == -1 and b"null" in L.lbm_last_error()
    assert L.lbm_debug_wall_rule(1, 2, -0.999, 1, f, out) == 0
    with pytest.raises(ValueError):
        lbm.debug_wall_rule("east", "no-slip", 0.0, [0.1] * 9)
    with pytest.raises(ValueError):
        lbm.debug_wall_rule("south", "sticky", 0.0, [0.1] * 9)


@pytest.mark.parametrize("args", [["--wall-south", "sticky"], ["--walls", "moving:nan"], ["--walls", "moving:1.5"],
                                  ["--wall-north", "moving:"], ["--wall-north", "moving:0.1x"], ["--wall-south", "moving:-1"],
                                  ["--walls"]])
def test_lbm_solver_refuses_bad_walls_before_it_touches_a_device(solver, tmp_path, args):
    pr = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 2, (pr.returncode, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and args[0] in lines[0], pr.stderr
    assert pr.stdout == ""
