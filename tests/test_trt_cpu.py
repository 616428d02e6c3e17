"""Two-relaxation-time (TRT) collision, the parts that need no GPU: the library exports lbm_set_trt, lbm_solver documents --trt-magic
and refuses a bad value (or --smagorinsky beside it) before any device is touched, and the plan candidates of a TRT context name
the TRT kernels and leave out the tall fp32 regions (which have no TRT instantiation)."""
import ctypes
import os
import subprocess

import pytest

from tests.helpers import lbm_cpu, solver  # noqa: F401


def test_library_exports_lbm_set_trt(lbm):
    L = lbm.lib()
    assert hasattr(L, "lbm_set_trt")
    assert L.lbm_set_trt.argtypes == [ctypes.c_void_p, ctypes.c_double]


def test_help_names_trt_magic(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "--trt-magic LAMBDA" in pr.stdout and "two-relaxation-time" in pr.stdout


def refused(solver, tmp_path, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    assert "--trt-magic" in pr.stderr and "unknown option" not in pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)


@pytest.mark.parametrize("value", ["-0.1", "nan", "abc", "2", "inf", "0.1x", ""])
def test_bad_trt_magic_exits_2_before_a_device_opens(solver, tmp_path, value):
    refused(solver, tmp_path, ["--trt-magic", value])


def test_smagorinsky_with_trt_magic_exits_2(solver, tmp_path):
    refused(solver, tmp_path, ["--smagorinsky", "0.17", "--trt-magic", "0.25"])


def candidates(lbm, precision, arith):
    L = lbm.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    L.lbm_debug_plan_candidates.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    assert L.lbm_debug_plan_candidates(4096, 1024, precision, arith, 256, buf, len(buf)) == 0
    return [line.split("|") for line in buf.value.decode().splitlines()]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("arith", [0, 1])
def test_trt_plan_candidates(lbm, precision, arith):
    bgk = candidates(lbm, precision, arith)
    trt = candidates(lbm, precision, arith + 4)
    tall = [c for c in bgk if "deep=8" in c[1]]
    assert bool(tall) == (precision == 1)                  # fp32 BGK measures the tall regions ...
    assert trt and not [c for c in trt if "deep=8" in c[1]]        # ... a TRT context does not
    assert [c for c in bgk if "deep=8" not in c[1]] == [c[:2] + [c[2][:-2] + "%d>" % arith] + c[3:] for c in trt]
    assert all(c[2].endswith(",%d>" % (arith + 4)) for c in trt)
