"""Per-row inlet profiles, the parts that need no GPU: the library exports lbm_set_inlet_profile, lbm_solver documents
--inlet-profile and refuses a bad profile file before any device is touched, and the Python helper parabolic_profile is exactly
the profile the CLI builds (lbm_solver --print-inlet-profile prints it without opening a device)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import lbm_cpu, solver  # noqa: F401


def run_solver(solver, cwd, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")   # (a device opened anyway would fail differently: "lbm_create" / "no HIP device")
    return subprocess.run([solver, "--steps", "1", "--no-vtk"] + [str(a) for a in args], cwd=cwd, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=60, env=env)


def printed_profile(pr):
    assert pr.returncode == 0, pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout
    return np.array([float(v) for v in pr.stdout.split()])


def test_library_exports_lbm_set_inlet_profile(lbm):
    L = lbm.lib()
    assert hasattr(L, "lbm_set_inlet_profile")
    assert L.lbm_set_inlet_profile.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]


def test_help_names_inlet_profile(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "--inlet-profile parabolic|FILE" in pr.stdout and "mean" in pr.stdout


@pytest.mark.parametrize("name,text,ny,why", [
    ("count", "1\n2\n3\n", 4, "3 values, the lattice has ny = 4 rows"),
    ("too-many", "1 2 3 4 5\n", 4, "5 values"),
    ("non-number", "1\n2\nthree\n4\n", 4, "line 3: 'three' is not a number"),
    ("trailing-garbage", "1\n2x\n3\n4\n", 4, "'2x' is not a number"),
    ("nan", "1\nnan\n3\n4\n", 4, "'nan' is not finite"),
    ("inf", "1\n2\n3\ninf\n", 4, "'inf' is not finite"),
    ("mean-zero", "1\n-1\n2\n-2\n", 4, "mean of the shape must be positive"),
    ("mean-negative", "-1\n-1\n0\n0\n", 4, "mean of the shape must be positive"),
    ("too-fast", "# one row carries it all\n0\n0\n0\n100\n", 4, "row 3 scales to"),
])
def test_malformed_profile_is_refused_before_any_device(solver, tmp_path, name, text, ny, why):
    p = tmp_path / f"{name}.txt"
    p.write_text(text)
    # inlet velocity 0.3: the "too-fast" shape puts 4 x 0.3 = 1.2 on its last row
    pr = run_solver(solver, tmp_path, "--nx", 16, "--ny", ny, "--inlet-velocity", 0.3, "--inlet-profile", p)
    assert pr.returncode == 2, (pr.returncode, pr.stderr)
    assert why in pr.stderr, pr.stderr
    assert "lbm_create" not in pr.stderr and "HIP" not in pr.stderr and "MI355X HIP Grid" not in pr.stdout


def test_missing_profile_file_is_refused(solver, tmp_path):
    pr = run_solver(solver, tmp_path, "--nx", 16, "--ny", 4, "--inlet-profile", tmp_path / "nope.txt")
    assert pr.returncode == 2 and "cannot open inlet profile" in pr.stderr


@pytest.mark.parametrize("ny,u", [(1, 0.05), (8, 0.02), (64, 0.04), (97, 0.013333), (1024, 0.1)])
def test_parabolic_profile_is_what_the_cli_builds(lbm, solver, tmp_path, ny, u):
    pr = run_solver(solver, tmp_path, "--nx", 16, "--ny", ny, "--inlet-velocity", u, "--inlet-profile", "parabolic",
                    "--print-inlet-profile")
    cli = printed_profile(pr)
    py = lbm.parabolic_profile(ny, u)
    assert cli.shape == (ny,) and np.array_equal(cli, py)          # %.17g round-trips a double exactly
    assert abs(float(np.mean(py)) - u) <= 1e-15 * ny * u           # the mean is the inlet velocity, to rounding
    s = (np.arange(ny) + 0.5) / ny
    assert np.allclose(py, s * (1 - s) * 6 * u * ny * ny / (ny * ny + 0.5), rtol=1e-12, atol=0)   # the parabola, mean u
    if ny > 1:
        assert np.allclose(py, py[::-1], rtol=1e-14, atol=0)        # symmetric about the channel's centre line


def test_profile_file_is_scaled_like_the_python_helper(lbm, solver, tmp_path):
    ny, u = 40, 0.03
    shape = np.linspace(-0.2, 1.0, ny) ** 2
    lines = ["# a shape, row 0 first", ""] + [repr(float(v)) for v in shape[:20]] + ["", " ".join(repr(float(v)) for v in shape[20:]) + "  # rest"]
    (tmp_path / "shape.txt").write_text("\n".join(lines) + "\n")
    cli = printed_profile(run_solver(solver, tmp_path, "--nx", 16, "--ny", ny, "--inlet-velocity", u, "--inlet-profile",
                                     tmp_path / "shape.txt", "--print-inlet-profile"))
    assert np.array_equal(cli, lbm.scale_inlet_profile(shape, u))
    # --reynolds sets the mean velocity first; the profile is scaled to it
    re = 20.0
    cli = printed_profile(run_solver(solver, tmp_path, "--nx", 16, "--ny", ny, "--reynolds", re, "--inlet-profile", "parabolic",
                                     "--print-inlet-profile"))
    assert np.array_equal(cli, lbm.parabolic_profile(ny, re * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * ny)))


def test_python_helpers_refuse_bad_shapes(lbm):
    with pytest.raises(ValueError):
        lbm.scale_inlet_profile([1.0, -1.0], 0.05)
    with pytest.raises(ValueError):
        lbm.scale_inlet_profile([0.0, 0.0, 1.0], 0.5)
