"""The uniform driving force (lbm_set_forcing, Guo's scheme), the parts that need no GPU: the library's symbols, lbm_solver's --forcing,
the forced model's build units and plan candidates, and the numpy reference operator of tests/forcing_reference.py — its own
conservation properties and a physics check, so that the GPU parity of tests/test_gpu_forcing.py means something."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle, make_params
from tests.forcing_reference import forcing_constants, guo_collide, guo_source
from tests.helpers import PKG, lbm_cpu, record, solver  # noqa: F401
from tests.reference import CX, CY, feq, oracle_run
from tests.test_trt_cpu import candidates


# ---- the library and the command line -------------------------------------------------------------------------------------------
def test_library_exports_the_two_symbols(lbm):
    L = lbm.lib()
    assert hasattr(L, "lbm_set_forcing") and hasattr(L, "lbm_get_forcing")
    assert L.lbm_set_forcing.argtypes == [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    fx, fy = ctypes.c_double(), ctypes.c_double()
    assert L.lbm_set_forcing(None, 1e-5, 0.0) == -1 and b"lbm_set_forcing: null context" in L.lbm_last_error()
    assert L.lbm_get_forcing(None, ctypes.byref(fx), ctypes.byref(fy)) == -1 and b"lbm_get_forcing: null context" in L.lbm_last_error()


def test_help_documents_forcing(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "[--forcing FX,FY]" in pr.stdout and "--forcing FX,FY: a uniform driving force" in pr.stdout
    assert "Cannot be combined with --smagorinsky or --trt-magic" in pr.stdout


def refused(solver, tmp_path, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("--forcing"), pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)
    return lines[0]


@pytest.mark.parametrize("value, why", [("abc", "is not a pair FX,FY"), ("1e-5", "is not a pair FX,FY"), ("1e-5,0,0", "is not a pair FX,FY"),
                                        ("", "is not a pair FX,FY"), (",", "has no number FX"), ("1e-5,", "has no number FY"),
                                        (",1e-5", "has no number FX"), ("1e-5x,0", "has no number FX"), ("0,1e-5 ", "has no number FY"),
                                        (" 1e-5,0", "has no number FX"), ("nan,0", "not finite or not below 1"),
                                        ("0,inf", "not finite or not below 1"), ("1,0", "not finite or not below 1"),
                                        ("0,-1.5", "not finite or not below 1")])
def test_bad_forcing_exits_2_before_a_device_opens(solver, tmp_path, value, why):
    line = refused(solver, tmp_path, ["--forcing", value])
    assert why in line and "'%s'" % value in line, line


@pytest.mark.parametrize("other", [["--smagorinsky", "0.17"], ["--trt-magic", "0.25"]])
def test_forcing_with_another_collision_exits_2(solver, tmp_path, other):
    for args in (other + ["--forcing", "2e-5,-1e-5"], ["--forcing", "-2e-5,1e-5"] + other):
        line = refused(solver, tmp_path, args)
        assert "cannot be combined with " + other[0] in line, line


# ---- the build units and the plan candidates --------------------------------------------------------------------------------------
def forced_row(lbm):
    """(tall, park) of the forced row of collision_models, as the plan candidates of a large grid show them."""
    tall = any("deep=8" in c[1] for c in candidates(lbm, 1, 9))
    park = any(re.search(r"deep=1[01]\b", c[1]) for c in candidates(lbm, 0, 9))
    return tall, park


def test_forced_model_has_the_units_of_base_0(lbm):
    build = __import__(PKG + ".build", fromlist=["build"])
    assert 8 in build.COLLISION_BASES
    units = build.units("0123456789abcdef")
    assert len({obj for _, _, obj in units}) == len(units)

    def kinds(flag, base):
        out = set()
        for src, flags, obj in units:
            if "%s=%d" % (flag, base) in flags:
                out.add((src, tuple(f for f in flags if not f.startswith(flag + "=")), re.sub(r"_ar\d+", "", obj)))
        return out
    forced, bgk = kinds("-DLBM_AR_BASE", 8), kinds("-DLBM_AR_BASE", 0)
    assert forced == bgk and len(forced) == 3
    assert {src for src, _, _ in forced} == {"lbm_step_k.hip", "lbm_col.hip"}
    tall, park = forced_row(lbm)
    assert kinds("-DLBM_COL_PARK", 8) == ({("lbm_col.hip", (), "lbm_col_park.o")} if park else set())
    assert dict(build.COLLISION_MODELS)[8] == park
    # the tall fp32 objects are BGK's two alone, whatever the models: a row that granted them to the forced model would need a third
    assert not tall
    assert sorted(obj for _, flags, obj in units if any(f.startswith("-DLBM_COL_TALL=") for f in flags)) == ["lbm_col_tall_c.o", "lbm_col_tall_s.o"]


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("arith", [0, 1])
def test_forced_plan_candidates(lbm, precision, arith):
    tall, park = forced_row(lbm)
    bgk = candidates(lbm, precision, arith)
    forced = candidates(lbm, precision, arith + 8)

    def keep(c):
        return ("deep=8" not in c[1] or tall) and (not re.search(r"deep=1[01]\b", c[1]) or park)
    assert forced and all(c[2].endswith(",%d>" % (arith + 8)) for c in forced)
    assert [c for c in bgk if keep(c)] == [c[:2] + [c[2][:-2] + "%d>" % arith] + c[3:] for c in forced]


# ---- the numpy operator's own properties (derived, not measured) --------------------------------------------------------------------
def near_equilibrium(n, seed):
    """n cells: the equilibrium of a random density near 1 and a random velocity below 0.1, each population moved by up to 1e-3 of
    itself."""
    rng = np.random.default_rng(seed)
    r = 1.0 + 0.05 * (rng.random(n) - 0.5)
    ux, uy = 0.2 * (rng.random(n) - 0.5), 0.2 * (rng.random(n) - 0.5)
    usq = ux * ux + uy * uy
    return [feq(i, r, ux, uy, usq) * (1.0 + 1e-3 * (rng.random(n) - 0.5)) for i in range(9)]


def collide_cells(f, tau, force):
    """guo_collide's arithmetic on bare cells (the list of nine arrays): the operator without the oracle around it."""
    wp, gx, gy, hx, hy = forcing_constants(tau, force)
    r = np.zeros_like(f[0]); jx = np.zeros_like(f[0]); jy = np.zeros_like(f[0])
    for i in range(9):
        r = r + f[i]
        jx = jx + float(CX[i]) * f[i]
        jy = jy + float(CY[i]) * f[i]
    ux, uy = (jx + hx) / r, (jy + hy) / r
    usq = ux * ux + uy * uy
    s = guo_source(r, ux, uy, gx, gy)
    return [(f[i] - wp * (f[i] - feq(i, r, ux, uy, usq))) + s[i] for i in range(9)], s


@pytest.mark.parametrize("tau", [0.55, 0.8, 1.3])
@pytest.mark.parametrize("force", [(2e-5, -1e-5), (1e-3, 0.0), (0.0, -1e-3), (-7e-4, 7e-4)])
def test_source_sums_to_zero_and_adds_the_force_to_the_momentum(tau, force):
    f = near_equilibrium(4096, 5)
    out, s = collide_cells(f, tau, force)
    # sum_i w_i = 1, sum_i w_i c_i = 0, sum_i w_i c_i c_i = I/3: sum S = 3 g.(0 - u) + 9 u.g/3 = 0 in exact arithmetic; nine terms of
    # magnitude below 4 |g| (1 + |u|) w_i each rounded to 2^-53 relative, summed: below 1e-17 for |F| <= 1e-3
    assert float(np.max(np.abs(sum(s)))) <= 1e-17
    # BGK keeps rho u; the equilibrium is taken at (j + F/2)/rho, so relaxation moves the momentum by wp F/2, and the source's first
    # moment is (1 - wp/2) F: F in all. Rounding: the momentum sums of populations of magnitude below 0.5, a few 1e-16 absolute.
    dx = sum(float(CX[i]) * (out[i] - f[i]) for i in range(9))
    dy = sum(float(CY[i]) * (out[i] - f[i]) for i in range(9))
    assert float(np.max(np.abs(dx - force[0]))) <= 1e-15 and float(np.max(np.abs(dy - force[1]))) <= 1e-15
    assert float(np.max(np.abs(sum(out) - sum(f)))) <= 1e-15                      # mass


def test_zero_force_is_the_oracles_collision_bit_for_bit():
    """On a developed flow whose relaxed populations hold no zero: x + S with S = 0.0 keeps every bit of x unless x is -0."""
    kw = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
    _, fcur = oracle_run(96, 40, 60, 0, keep_f_current=True, **kw)
    outs = []
    for forced in (False, True):
        o = Oracle(make_params(96, 40, **kw))
        o.L.lbmo_initialise(o.h)
        o.f_current[:] = fcur
        if forced:
            guo_collide(o, o.p.tau, (0.0, 0.0))
        else:
            o.collide()
        assert np.all(o.f_next[1:-1, 1:-1][~o.solid.astype(bool)] != 0.0)
        outs.append((o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy()))
        o.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- a physics check of the reference ----------------------------------------------------------------------------------------------
def test_force_replaces_the_pressure_gradient_of_a_channel(lbm):
    """Poiseuille flow between the two walls, fed its own parabola at the inlet. Unforced, the density falls along the channel as the
    pressure gradient dp/dx = -8 nu u_max / H^2 that drives the parabola asks; with Fx = 8 nu u_max / H^2 the force drives it and the
    density stays flat. The ratio of the two drops along the centre line, measured on the reference here (recorded below): 0.0850 at
    these parameters (0.0830 after 6000 steps; 0.058 at 128x32: the on-node walls stand half a cell inside the H = ny the profile
    assumes, so the force is (23 / 24)^2, about 8 %, short of what that narrower channel needs, and the unforced drop is 15 % above the expected one for
    the same reason). Asserted with a margin of two over that."""
    nx, ny, steps, tau = 96, 24, 2500, 0.8
    u = lbm.parabolic_profile(ny, 0.04)
    nu, u_max, H = (tau - 0.5) / 3.0, float(np.max(u)), float(ny)
    fx = 8.0 * nu * u_max / (H * H)
    mask = np.zeros((ny, nx), np.uint8)
    drops = []
    for force in (None, (fx, 0.0)):
        run = oracle_run(nx, ny, steps, 0, mask=mask, u=u, tau=tau, inlet_velocity=0.04,
                         collide=None if force is None else functools.partial(guo_collide, force=force))
        assert run.first_unstable == -1
        drops.append(float(run.rho[ny // 2, nx // 4] - run.rho[ny // 2, 3 * nx // 4]))
    expected = 3.0 * fx * (3 * nx // 4 - nx // 4)             # rho = 3 p: the drop the gradient asks for over the stretch
    ratio = abs(drops[1]) / abs(drops[0])
    record("forcing_channel_density_drop", unforced=drops[0], forced=drops[1], ratio=ratio, expected_unforced=expected)
    assert 0.5 * expected <= drops[0] <= 1.5 * expected, (drops, expected)        # the unforced run is the Poiseuille flow meant
    assert ratio <= 2 * 0.0850, (drops, ratio)
