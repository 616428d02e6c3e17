"""The inlet schedule of lbm_set_inlet_schedule without a GPU: oracle_run(schedule=...) pinned to oracle_run(u=...), the index
function the kernels call (lbm_debug_inlet_scale: compiled for the host) against a Python restatement, the argument errors that need
no device (the library's and lbm_solver's), and the C++ builders of --inlet-ramp / --inlet-pulse against the Python helpers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.helpers import lbm_cpu, masks, solver  # noqa: F401
from tests.reference import HOLD, REPEAT, oracle_run, sched_index

MAX = 1048576       # LBM_INLET_SCHEDULE_MAX


def same_run(a, b):
    assert a.first_unstable == b.first_unstable == -1 and a.solid_count == b.solid_count
    for name in ("f_next", "rho", "ux", "uy"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.forces == b.forces


# ---- schedule= against u= --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1.0, 0.7, -0.4])
def test_a_constant_schedule_is_the_scaled_profile_bit_for_bit(c):
    nx, ny, steps, of = 96, 40, 45, 10
    kw = dict(inlet_velocity=0.05)
    y = (np.arange(ny) + 0.5) / ny
    u = 0.3 * y * (1 - y) * (1.0 + 0.3 * np.sin(1.7 * np.arange(ny)))
    mask = masks(200, 64)["inlet-outlet"][:ny, :nx]
    for mode in (HOLD, REPEAT):
        same_run(oracle_run(nx, ny, steps, of, schedule=([c], mode), mask=mask, u=u, **kw), oracle_run(nx, ny, steps, of, mask=mask, u=c * u, **kw))
    # without a profile: the uniform inlet_velocity on every row
    same_run(oracle_run(nx, ny, steps, of, schedule=([c, c, c], HOLD), **kw), oracle_run(nx, ny, steps, of, u=c * np.full(ny, 0.05), **kw))


def test_a_varying_schedule_changes_the_run_and_reports_the_last_factor():
    nx, ny, steps = 96, 40, 23
    u = np.full(ny, 0.05)
    s = 1.0 + 0.5 * np.sin(2 * np.pi * np.arange(7) / 7)
    a = oracle_run(nx, ny, steps, 0, schedule=(s, REPEAT), inlet_velocity=0.05)
    b = oracle_run(nx, ny, steps, 0, u=u, inlet_velocity=0.05)
    assert not np.array_equal(a.f_next, b.f_next)
    assert np.array_equal(a.ux[:, 0], u * s[(steps - 1) % 7])


# ---- the index function -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mode", [HOLD, REPEAT])
@pytest.mark.parametrize("n", [1, 2, 7, 200, MAX])
def test_inlet_scale_hook_against_the_restatement(lbm, n, mode, precision):
    rng = np.random.default_rng(n + mode)
    s = rng.standard_normal(n) * 1.5 + 1.0 / 3.0         # (entries that fp32 rounds)
    t = sorted({0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n, 3 * n + 5, 2 ** 31 - 1} - {-1})
    got = lbm.debug_inlet_scale(s, mode, t, precision)
    T = np.float64 if precision == "f64" else np.float32
    want = np.array([float(T(s[sched_index(k, n, mode)])) for k in t])
    assert np.array_equal(got, want)
    if precision == "f32":
        assert not np.array_equal(got, np.array([s[sched_index(k, n, mode)] for k in t]))
    if n > 1:       # HOLD clamps and REPEAT wraps: the two differ past the end
        assert got[t.index(n)] == float(T(s[n - 1] if mode == HOLD else s[0]))
        assert got[-1] == float(T(s[n - 1] if mode == HOLD else s[(2 ** 31 - 1) % n]))
    assert np.array_equal(lbm.debug_inlet_scale(s, ("hold", "repeat")[mode], t, precision), got)


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_schedule_argument_errors_without_a_device(lbm):
    L = lbm.lib()
    s = (C.c_double * 4)(0.0, 0.5, 1.0, 1.0)
    t = (C.c_int * 2)(0, 5)
    out = (C.c_double * 2)()
    v = C.c_double()
    assert L.lbm_set_inlet_schedule(None, s, 4, 0) == -1 and b"null context" in L.lbm_last_error()
    assert L.lbm_inlet_schedule_length(None) == 0
    assert L.lbm_get_inlet_scale(None, 0, C.byref(v)) == -1 and b"null" in L.lbm_last_error()
    # the checks lbm_set_inlet_schedule shares with the hook (the GPU file runs them on a context)
    for args, text in (((s, -1, 0), b"n = -1"), ((s, MAX + 1, 0), b"n = 1048577"), ((None, 3, 0), b"null table"),
                       ((s, 4, 2), b"mode = 2"), ((s, 4, -1), b"mode = -1")):
        assert L.lbm_debug_inlet_scale(args[0], args[1], args[2], 0, t, 2, out) == -1, args[1:]
        assert text in L.lbm_last_error(), (args[1:], L.lbm_last_error())
    for bad in (float("nan"), float("inf"), -float("inf")):
        b = (C.c_double * 4)(0.0, 0.5, bad, 1.0)
        assert L.lbm_debug_inlet_scale(b, 4, 1, 0, t, 2, out) == -1 and b"entry 2" in L.lbm_last_error()
    assert L.lbm_debug_inlet_scale(s, 4, 0, 2, t, 2, out) == -1 and b"precision" in L.lbm_last_error()
    assert L.lbm_debug_inlet_scale(s, 4, 0, 0, None, 2, out) == -1 and b"null" in L.lbm_last_error()
    assert L.lbm_debug_inlet_scale(s, 0, 0, 0, t, 2, out) == -1 and b"n = 0" in L.lbm_last_error()
    neg = (C.c_int * 2)(3, -1)
    assert L.lbm_debug_inlet_scale(s, 4, 0, 0, neg, 2, out) == -1 and b"t[1] = -1" in L.lbm_last_error()
    assert L.lbm_debug_inlet_scale(s, 4, 0, 1, t, 2, out) == 0 and list(out) == [0.0, 1.0]
    with pytest.raises(ValueError):
        lbm.debug_inlet_scale([1.0], "sometimes", [0])
    with pytest.raises(ValueError):
        lbm.cosine_ramp(0)
    with pytest.raises(ValueError):
        lbm.sine_pulse(0.5, 0)


def test_the_helpers_are_what_they_say(lbm):
    r = lbm.cosine_ramp(22)
    assert r.shape == (23,) and r[0] == 0.0 and abs(r[-1] - 1.0) <= 1e-16 and np.all(np.diff(r) > 0)
    assert np.array_equal(r, np.array([0.5 * (1.0 - np.cos(np.pi * k / 22)) for k in range(23)]))
    p = lbm.sine_pulse(0.5, 7)
    assert p.shape == (7,) and p[0] == 1.0 and abs(np.mean(p) - 1.0) < 1e-15
    assert np.array_equal(p, np.array([1.0 + 0.5 * np.sin(2.0 * np.pi * k / 7) for k in range(7)]))


# ---- lbm_solver: the builders and the refusals ------------------------------------------------------------------------------------
def printed(solver, tmp_path, args):
    pr = subprocess.run([solver] + args + ["--print-inlet-schedule"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        text=True, timeout=60)
    assert pr.returncode == 0, pr.stderr
    return np.array([float(l) for l in pr.stdout.split()])


def ulps(a, b):
    return np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b))))


def test_print_inlet_schedule_against_the_helpers(lbm, solver, tmp_path):
    # libm and numpy may differ in the last bit of cos / sin: one ulp for the two builders, bits for a file
    for n in (1, 22, 150):
        got, want = printed(solver, tmp_path, ["--inlet-ramp", str(n)]), lbm.cosine_ramp(n)
        assert got.shape == want.shape == (n + 1,) and ulps(got, want) <= 1.0, n
    for a, p in ((0.5, 7), (-0.3, 200), (1.25, 1)):
        got, want = printed(solver, tmp_path, ["--inlet-pulse", f"{a}:{p}"]), lbm.sine_pulse(a, p)
        assert got.shape == want.shape == (p,) and ulps(got, want) <= 1.0, (a, p)
    s = np.random.default_rng(5).standard_normal(37)
    (tmp_path / "s.txt").write_text("# a schedule\n" + "\n".join(repr(float(v)) for v in s[:20]) + " # half\n\n" +
                                    " ".join(repr(float(v)) for v in s[20:]) + "\n")
    assert np.array_equal(printed(solver, tmp_path, ["--inlet-schedule", str(tmp_path / "s.txt")]), s)
    assert np.array_equal(printed(solver, tmp_path, ["--inlet-schedule", str(tmp_path / "s.txt"), "--inlet-schedule-repeat"]), s)


@pytest.mark.parametrize("args,text", [
    (["--inlet-ramp", "0"], "--inlet-ramp"), (["--inlet-ramp", "1e3"], "--inlet-ramp"), (["--inlet-ramp", "1048576"], "--inlet-ramp"),
    (["--inlet-ramp"], "--inlet-ramp"), (["--inlet-pulse", "0.5"], "--inlet-pulse"), (["--inlet-pulse", "x:7"], "--inlet-pulse"),
    (["--inlet-pulse", "nan:7"], "--inlet-pulse"), (["--inlet-pulse", "0.5:0"], "--inlet-pulse"),
    (["--inlet-pulse", "0.5:1048577"], "--inlet-pulse"), (["--inlet-ramp", "5", "--inlet-pulse", "0.5:7"], "cannot be combined"),
    (["--inlet-pulse", "0.5:7", "--inlet-schedule", "s.txt"], "cannot be combined"),
    (["--inlet-schedule", "s.txt", "--inlet-ramp", "5"], "cannot be combined"),
    (["--inlet-schedule", "missing.txt"], "missing.txt"), (["--inlet-schedule", "empty.txt"], "0 values"),
    (["--inlet-schedule", "word.txt"], "not a number"), (["--inlet-schedule", "inf.txt"], "not finite"),
    (["--inlet-ramp", "5", "--inlet-schedule-repeat"], "--inlet-schedule-repeat"), (["--print-inlet-schedule"], "--print-inlet-schedule"),
    (["--inlet-schedule", "big.txt"], "entry 1"), (["--inlet-schedule", "big.txt", "--inlet-profile", "parabolic"], "row"),
    (["--inlet-pulse", "30:4", "--inlet-velocity", "0.05"], "entry 1")])
def test_lbm_solver_refuses_bad_schedules_before_it_touches_a_device(solver, tmp_path, args, text):
    (tmp_path / "s.txt").write_text("0 0.5 1\n")
    (tmp_path / "empty.txt").write_text("# nothing\n")
    (tmp_path / "word.txt").write_text("0 half 1\n")
    (tmp_path / "inf.txt").write_text("0 inf 1\n")
    (tmp_path / "big.txt").write_text("1 100 1\n")          # 0.01333 * 100 >= 1: the inlet divides by 1 - u s
    pr = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 2, (pr.returncode, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and text in lines[0], pr.stderr
    assert pr.stdout == ""


def test_the_header_declares_the_schedule(lbm):
    from tests.test_cabi_cpu import declared_symbols
    names = set(declared_symbols())
    assert {"lbm_set_inlet_schedule", "lbm_inlet_schedule_length", "lbm_get_inlet_scale", "lbm_debug_inlet_scale"} <= names
    for n in ("lbm_set_inlet_schedule", "lbm_inlet_schedule_length", "lbm_get_inlet_scale", "lbm_debug_inlet_scale"):
        assert getattr(lbm.lib(), n)
