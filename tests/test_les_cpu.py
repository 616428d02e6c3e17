"""Smagorinsky LES collision, the parts that need no GPU: the library exports lbm_set_smagorinsky, lbm_solver documents
--smagorinsky and refuses a bad value before any device is touched, and the plan candidates of an LES context name the LES
kernels and leave out the tall fp32 regions (which have no LES instantiation)."""
import ctypes
import os
import subprocess

import pytest

from tests.helpers import lbm_cpu, solver  # noqa: F401


def test_library_exports_lbm_set_smagorinsky(lbm):
    L = lbm.lib()
    assert hasattr(L, "lbm_set_smagorinsky")
    assert L.lbm_set_smagorinsky.argtypes == [ctypes.c_void_p, ctypes.c_double]


def test_help_names_smagorinsky(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "--smagorinsky CS" in pr.stdout and "molecular viscosity" in pr.stdout


@pytest.mark.parametrize("value", ["-0.1", "nan", "abc", "2", "inf", "0.1x", ""])
def test_bad_smagorinsky_exits_2_before_a_device_opens(solver, tmp_path, value):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk", "--smagorinsky", value], cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    assert "--smagorinsky" in pr.stderr and "unknown option" not in pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)


def candidates(lbm, precision, arith):
    L = lbm.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    L.lbm_debug_plan_candidates.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    assert L.lbm_debug_plan_candidates(4096, 1024, precision, arith, 256, buf, len(buf)) == 0
    return [line.split("|") for line in buf.value.decode().splitlines()]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("arith", [0, 1])
def test_les_plan_candidates(lbm, precision, arith):
    bgk = candidates(lbm, precision, arith)
    les = candidates(lbm, precision, arith + 2)
    tall = [c for c in bgk if "deep=8" in c[1]]
    assert bool(tall) == (precision == 1)                  # fp32 BGK measures the tall regions ...
    assert not [c for c in les if "deep=8" in c[1]]        # ... an LES context does not
    assert [c for c in bgk if "deep=8" not in c[1]] == [c[:2] + [c[2][:-2] + "%d>" % arith] + c[3:] for c in les]
    assert all(c[2].endswith(",%d>" % (arith + 2)) for c in les)
