"""The outlet sponge (lbm_set_sponge), the parts that need no GPU: the numpy reference of tests/sponge_reference.py against plain BGK,
so that the GPU parity of tests/test_gpu_sponge.py means something; the setter and its refusals through the library's device-less
hooks; the rates lbm_get_sponge_rate reports; the table's row (plan candidates, kernel names, withheld shapes, launchers); checkpoint
heads; the dry-run choreography; lbm_solver's --sponge; and one physical check that the sponge lowers what comes back from the outlet."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import PKG, lbm_cpu, record, solver  # noqa: F401
from tests.reference import oracle_run
from tests.sponge_reference import R_NX, R_NY, R_STEPS, R_TAU_END, R_W, collide_of, reflection_pair, sponge_rates
from tests.test_ckpt_cpu import MASK_D, PROFILE_D, SCHED_D, WALLS, describe
from tests.test_choreography_cpu import dry  # noqa: F401
from tests.test_mrt_cpu import FORCING, INITIALISE_DEEP, INITIALISED, LES, MRT, TRT, setters
from tests.test_trt_cpu import candidates

SPONGE = 6                                  # lbm_debug_collision_setters: lbm_set_sponge((int)v1, v2)
SPONGE_BASE, SPONGE_BIT = 32, 2048
NOUN = "outlet sponge"


# ---- 1. the reference against plain BGK -----------------------------------------------------------------------------------------------
def test_tau_end_equal_to_tau_is_plain_bgk_bit_for_bit():
    kw = dict(tau=0.53, inlet_velocity=0.08, cylinder_radius=0.1)
    plain = oracle_run(200, 40, 40, 10, **kw)
    same = oracle_run(200, 40, 40, 10, collide=collide_of(48, kw["tau"]), **kw)
    assert plain.first_unstable == same.first_unstable == -1
    assert np.array_equal(plain.f_next, same.f_next) and plain.forces == same.forces
    for a, b in ((plain.rho, same.rho), (plain.ux, same.ux), (plain.uy, same.uy)):
        assert np.array_equal(a, b)


def test_columns_the_zone_has_not_reached_equal_the_plain_run():
    """Information travels one column per iteration: after n iterations every column x <= x0 - n is plain BGK's bit for bit, and the zone
    itself is not (the operator is active)."""
    nx, ny, width, n = 200, 40, 48, 40
    kw = dict(tau=0.53, inlet_velocity=0.08, cylinder_radius=0.1)
    plain = oracle_run(nx, ny, n, 0, **kw)
    sponge = oracle_run(nx, ny, n, 0, collide=collide_of(width, 1.5), **kw)
    x0 = nx - 1 - width
    hi = x0 - n + 2                                         # columns 0 .. x0 - n of the ghost-inclusive array, its west ghost column too
    assert hi > 100 and np.array_equal(plain.f_next[:, :hi], sponge.f_next[:, :hi])
    assert not np.array_equal(plain.f_next[:, x0 + 2:], sponge.f_next[:, x0 + 2:])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_rates_are_bgks_outside_the_zone(dtype):
    tau = 0.55
    wp = sponge_rates(160, tau, 48, 1.5, dtype)
    assert wp.dtype == dtype and np.all(wp[:112] == dtype(1.0 / tau)) and np.all(np.diff(wp[111:].astype(np.float64)) < 0.0)
    assert wp[159] == dtype(1.0 / 1.5)


# ---- 2. the setter and its refusals, without a device -----------------------------------------------------------------------------------
def test_library_exports_the_three_symbols(lbm):
    L = lbm.lib()
    assert L.lbm_set_sponge.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double]
    w, t, r = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    assert L.lbm_set_sponge(None, 48, 1.5) == -1 and b"lbm_set_sponge: null context" in L.lbm_last_error()
    assert L.lbm_get_sponge(None, ctypes.byref(w), ctypes.byref(t)) == -1 and b"lbm_get_sponge: null context" in L.lbm_last_error()
    assert L.lbm_get_sponge_rate(None, 0, ctypes.byref(r)) == -1 and b"lbm_get_sponge_rate: null context" in L.lbm_last_error()


def test_set_get_and_clear(lbm):
    for width, tau_end in ((1, 1.5), (63, 0.500001), (20, 0.52), (48, 1e300)):
        out, state = setters(lbm, [(SPONGE, width, tau_end)])
        assert out == [(0, "")] and state[0] == SPONGE_BASE, (width, tau_end, out)
        assert lbm.debug_sponge_rates(64, 0.55, "f64", width, tau_end)[0] == (width, tau_end)
    # width == 0 clears the model, whatever tau_end; on a context without it nothing changes
    for calls in ([(SPONGE, 48, 1.5), (SPONGE, 0, 1.5)], [(SPONGE, 0, 0.0)], [(SPONGE, 0, float("nan"))], [(SPONGE, 48, 1.5), (SPONGE, 0, -7.0)]):
        out, state = setters(lbm, calls)
        assert all(rc == 0 for rc, _ in out) and state[0] == 0, (calls, out, state)
    assert lbm.debug_sponge_rates(64, 0.55, "f64", 0, 1.5)[0] == (0, 0.0)
    out, state = setters(lbm, [(TRT, 0.25, 0.0), (SPONGE, 0, 0.0)])            # clearing the sponge leaves another model alone
    assert out == [(0, ""), (0, "")] and state[0] == 4


@pytest.mark.parametrize("width, tau_end, text", [
    (-1, 1.5, "lbm_set_sponge: width = -1 (0 .. nx - 1 = 63 only: column 0 keeps tau)"),
    (64, 1.5, "lbm_set_sponge: width = 64 (0 .. nx - 1 = 63 only: column 0 keeps tau)"),
    (48, float("nan"), "lbm_set_sponge: tau_end = nan (finite values above 0.5 only)"),
    (48, float("inf"), "lbm_set_sponge: tau_end = inf (finite values above 0.5 only)"),
    (48, 0.5, "lbm_set_sponge: tau_end = 0.5 (finite values above 0.5 only)"),
    (48, -1.5, "lbm_set_sponge: tau_end = -1.5 (finite values above 0.5 only)"),
])
def test_bad_values_are_refused_by_name(lbm, width, tau_end, text):
    out, state = setters(lbm, [(SPONGE, width, tau_end)])
    assert out == [(-1, text)] and state[0] == 0


def test_tau_and_initialised_context_are_refused(lbm):
    for tau in (0.5, 0.3):
        out, state = setters(lbm, [(SPONGE, 48, 1.5)], tau=tau)
        assert out == [(-1, "lbm_set_sponge: tau = %g (the sponge's rates need tau > 0.5)" % tau)] and state[0] == 0
        assert setters(lbm, [(SPONGE, 0, 1.5)], tau=tau)[0] == [(0, "")]
    out, state = setters(lbm, [(SPONGE, 48, 1.5), (INITIALISED, 0, 0), (SPONGE, 20, 1.5), (SPONGE, 0, 0.0)])
    assert out[2] == out[3] == (-1, "lbm_set_sponge must be called before lbm_initialise") and state[0] == SPONGE_BASE


OTHERS = [(LES, 0.17, 0.0, "lbm_set_smagorinsky: Cs = 0.17", "Smagorinsky constant Cs = 0.17", 2),
          (TRT, 0.25, 0.0, "lbm_set_trt: magic parameter 0.25", "TRT magic parameter 0.25", 4),
          (FORCING, 2e-5, -1e-5, "lbm_set_forcing: force (2e-05, -1e-05)", "forcing F = (2e-05, -1e-05)", 8),
          (MRT, 1.0, 0.1875, "lbm_set_mrt: (bulk rate, magic) = (1, 0.1875)", "MRT parameters (bulk rate, magic) = (1, 0.1875)", 16)]
SPONGE_HAS = "sponge (width, tau_end) = (48, 1.5)"


@pytest.mark.parametrize("which, v1, v2, sets, has, base", OTHERS)
def test_mutual_exclusion_in_both_orders(lbm, which, v1, v2, sets, has, base):
    out, state = setters(lbm, [(which, v1, v2), (SPONGE, 48, 1.5)])
    assert out[0] == (0, "") and state[0] == base
    assert out[1] == (-1, "lbm_set_sponge: (width, tau_end) = (48, 1.5) on a context with %s (the two collisions cannot be combined)" % has)
    out, state = setters(lbm, [(SPONGE, 48, 1.5), (which, v1, v2)])
    assert out[0] == (0, "") and state[0] == SPONGE_BASE
    assert out[1] == (-1, "%s on a context with %s (the two collisions cannot be combined)" % (sets, SPONGE_HAS))
    # either model cleared, the other is taken
    out, state = setters(lbm, [(SPONGE, 48, 1.5), (SPONGE, 0, 0.0), (which, v1, v2)])
    assert [rc for rc, _ in out] == [0, 0, 0] and state[0] == base
    out, state = setters(lbm, [(which, v1, v2), (which, 0.0, 0.0), (SPONGE, 48, 1.5)])
    assert [rc for rc, _ in out] == [0, 0, 0] and state[0] == SPONGE_BASE


# ---- 3. the rates the kernels see -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("nx, width", [(160, 48), (150, 1), (150, 149), (70, 37), (40, 20), (260, 130), (2, 1)])
def test_rates_are_sponge_tau_cast_once(lbm, precision, nx, width):
    tau, tau_end = 0.55, 1.5
    dtype = np.float32 if precision == "f32" else np.float64
    pair, got = lbm.debug_sponge_rates(nx, tau, precision, width, tau_end)
    want = (1.0 / lbm.sponge_tau(nx, tau, width, tau_end)).astype(dtype).astype(np.float64)
    assert pair == (width, tau_end) and np.array_equal(got, want)
    x0 = nx - 1 - width
    bgk = float(dtype(1.0 / tau))
    assert np.all(got[:x0 + 1] == bgk) and got[x0] == bgk                  # column x0 and everything west of it: BGK's bits
    assert np.all(got[x0 + 1:] < bgk) and got[nx - 1] == float(dtype(1.0 / tau_end))
    # without a sponge every column reports BGK's rate
    assert np.all(lbm.debug_sponge_rates(nx, tau, precision, 0, tau_end)[1] == bgk)


def test_sponge_tau_is_the_formula_of_the_header(lbm):
    nx, tau, width, tau_end = 200, 0.53, 48, 1.5
    t = lbm.sponge_tau(nx, tau, width, tau_end)
    x0 = nx - 1 - width
    for x in (0, x0, x0 + 1, x0 + 17, nx - 1):
        s = float(x - x0) / float(width)
        assert t[x] == (tau if x <= x0 else tau + (tau_end - tau) * (s * s))
    assert t[nx - 1] == tau_end and t.dtype == np.float64 and t.shape == (nx,)
    assert np.array_equal(lbm.sponge_tau(nx, tau, 0, tau_end), np.full(nx, tau))
    for bad in (-1, nx):
        with pytest.raises(ValueError):
            lbm.sponge_tau(nx, tau, bad, tau_end)


def test_refused_setter_raises_with_the_librarys_text(lbm):
    with pytest.raises(lbm.LbmError, match=r"lbm_set_sponge: width = 40 \(0 \.\. nx - 1 = 39 only: column 0 keeps tau\)"):
        lbm.debug_sponge_rates(40, 0.55, "f64", 40, 1.5)


# ---- 4. the table's row: plan candidates, kernel names, the shapes withheld, the launchers -----------------------------------------------
def sponge_row(lbm):
    """(tall, park) of the sponge's row of collision_models, as the plan candidates of a large grid show them."""
    tall = any("deep=8" in c[1] for c in candidates(lbm, 1, SPONGE_BASE + 1))
    park = any(re.search(r"deep=1[01]\b", c[1]) for c in candidates(lbm, 0, SPONGE_BASE + 1))
    return tall, park


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("arith", [0, 1])
def test_sponge_plan_candidates_and_kernel_names(lbm, precision, arith):
    tall, park = sponge_row(lbm)
    bgk = candidates(lbm, precision, arith)
    sponge = candidates(lbm, precision, arith + SPONGE_BASE)

    def keep(c):
        return ("deep=8" not in c[1] or tall) and (not re.search(r"deep=1[01]\b", c[1]) or park)
    assert sponge and all(c[2].endswith(",%d>" % (arith + SPONGE_BASE)) for c in sponge)
    assert [c for c in bgk if keep(c)] == [c[:2] + [c[2][:-len("%d>" % (arith + SPONGE_BASE))] + "%d>" % arith] + c[3:] for c in sponge]


def test_withheld_shapes_are_refused_with_the_tables_text(lbm):
    tall, park = sponge_row(lbm)
    if not tall:          # the fp32 64x48 regions: BGK's alone
        out, state = setters(lbm, [(SPONGE, 48, 1.5)], precision=1, options="tune=0 deep=8")
        assert out == [(-1, "deep 8 (64x48 regions in registers) has no %s kernel" % NOUN)] and state[0] == 0
    for deep in (10, 11):
        out, state = setters(lbm, [(SPONGE, 48, 1.5), (INITIALISE_DEEP, 0, 0)], options="tune=0 arith=1 deep=%d" % deep)
        if park:
            assert out == [(0, ""), (0, "")]
        else:
            assert out == [(-1, "deep %d (64x40 regions in registers) has no %s kernel" % (deep, NOUN)), (0, "")] and state[0] == 0
    for deep in (1, 2, 3, 6, 7, 9):      # the LDS tiles and the 64x32 regions every model has
        assert setters(lbm, [(SPONGE, 48, 1.5), (INITIALISE_DEEP, 0, 0)], options="tune=0 arith=1 deep=%d" % deep)[0] == [(0, ""), (0, "")]


def test_sponge_kernels_ride_in_bgks_objects(lbm):
    """The build list holds the models that have objects of their own; the sponge is BGK's code with another rate and is instantiated
    in BGK's objects (collision_models: unit). The library then defines the sponge launchers of every family (the register kernel's on
    the regions the row grants) and leaves none unresolved (tests/test_collision_units_cpu.py)."""
    build = __import__(PKG + ".build", fromlist=["build"])
    assert SPONGE_BASE not in build.COLLISION_BASES and 0 in build.COLLISION_BASES
    units = build.units("0123456789abcdef")
    assert not [obj for _, flags, obj in units if any(f.endswith("=%d" % SPONGE_BASE) for f in flags)]
    tall, park = sponge_row(lbm)
    out = subprocess.run(["nm", "-D", "--defined-only", "--demangle", build.build_all()], stdout=subprocess.PIPE, text=True, check=True,
                         timeout=60).stdout
    for t in ("double", "float"):
        for launcher in ("launch_site<%s, 32>", "launch_deep<%s, 32>", "launch_tile<%s, 32>", "launch_col<%s, 0, 32>", "launch_col<%s, 0, 33>"):
            assert "lbmk::" + launcher % t + "(" in out, launcher % t
    assert ("launch_col<double, 2, 33>" in out) == park
    assert ("launch_col<float, 1, 32>" in out) == tall and ("launch_col<float, 1, 33>" in out) == tall


# ---- 5. checkpoint heads ------------------------------------------------------------------------------------------------------------------
PAIR = (48.0, 1.5)
PORTS = (1.0, 1.004, 1.0, 0.996)


def sponge_head(lbm, params=PAIR, base=SPONGE_BASE, ports=False, periodic=False, **fields):
    d = describe(**fields)
    h = lbm.CkptHead(**d.fixed)
    h.has_mask, h.mask_digest = d.mask is not None, d.mask or 0
    h.has_profile, h.profile_digest = d.profile is not None, d.profile or 0
    h.has_sched, h.sched_digest = d.sched is not None, d.sched or 0
    if d.walls is not None:
        h.has_walls, h.walls = 1, (ctypes.c_double * 4)(*d.walls)
    if params is not None:
        h.collision, h.collision_param = base, (ctypes.c_double * 2)(*params)
    if ports:
        h.has_ports, h.ports = 1, (ctypes.c_double * 4)(*PORTS)
    h.has_periodic_y = 1 if periodic else 0
    return h


def test_checkpoint_head_carries_the_pair_behind_mrts_place(lbm):
    assert lbm.binding.CKPT_HEAD_MAX == 184                                  # (a head has one model: the layout keeps its size)
    data = lbm.debug_ckpt_save(sponge_head(lbm))
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (SPONGE_BIT,) + PAIR and len(data) == 96
    assert SPONGE_BIT > 1024                                                   # bit order: behind MRT's bit 10, the ports and periodic y
    data = lbm.debug_ckpt_save(sponge_head(lbm, ports=True, periodic=True))
    assert struct.unpack("<Q4ddd", data[72:128]) == (256 | 512 | SPONGE_BIT,) + PORTS + PAIR and len(data) == 128
    full = sponge_head(lbm, ports=True, periodic=True, mask=True, profile=True, walls=True, sched=True)
    data = lbm.debug_ckpt_save(full)
    assert len(data) == 184
    assert struct.unpack("<QQQ4dQ4ddd", data[72:184]) == (1 | 2 | 16 | 32 | 256 | 512 | SPONGE_BIT, MASK_D, PROFILE_D) + WALLS + (SCHED_D,) + PORTS + PAIR
    assert lbm.debug_ckpt_load(data, full) == 184 and lbm.debug_ckpt_load(data + bytes(100), full) == 184


def test_checkpoint_loads_only_into_an_equal_sponge(lbm):
    data = lbm.debug_ckpt_save(sponge_head(lbm))
    assert lbm.debug_ckpt_load(data, sponge_head(lbm)) == len(data)
    for other in ((47.0, 1.5), (48.0, 1.25)):
        with pytest.raises(lbm.LbmError, match=r"written with sponge \(width, tau_end\) = \(48, 1\.5\); this context has \(width, tau_end\) = \(%s, %s\)"
                           % tuple(re.escape("%.17g" % v) for v in other)):
            lbm.debug_ckpt_load(data, sponge_head(lbm, params=other))
    bgk = lbm.debug_ckpt_save(sponge_head(lbm, params=None))
    assert bgk[:8] == b"LBMCKPT1"
    with pytest.raises(lbm.LbmError, match=r"written without a sponge; this context has \(width, tau_end\) = \(48, 1\.5\)"):
        lbm.debug_ckpt_load(bgk, sponge_head(lbm))
    with pytest.raises(lbm.LbmError, match=r"written with sponge \(width, tau_end\) = \(48, 1\.5\); this context has none"):
        lbm.debug_ckpt_load(data, sponge_head(lbm, params=None))
    # an MRT file into a sponge context and the reverse: the sponge, the last row of the table, is named first
    mrt = sponge_head(lbm, params=(1.0, 0.1875), base=16)
    mrt_bytes = lbm.debug_ckpt_save(mrt)
    with pytest.raises(lbm.LbmError, match="written without a sponge"):
        lbm.debug_ckpt_load(mrt_bytes, sponge_head(lbm))
    with pytest.raises(lbm.LbmError, match="written with sponge"):
        lbm.debug_ckpt_load(data, mrt)
    # a head that announces two collision models is no checkpoint
    two = data[:72] + struct.pack("<Qdddd", 1024 | SPONGE_BIT, 1.0, 0.1875, *PAIR)
    with pytest.raises(lbm.LbmError):
        lbm.debug_ckpt_load(two, sponge_head(lbm))


# ---- 6. the dry-run choreography ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options, precision", [(dict(fuse=1), 0), (dict(fuse=3, pair_ty=12), 0), (dict(deep=1), 0), (dict(deep=7, arith=1), 0),
                                                (dict(deep=6), 1), (dict(deep=7, arith=1), 1)])
def test_choreography_is_that_of_bgk(dry, options, precision):  # noqa: F811
    for transport, bounds, ny in ((0, [(0, 44), (44, 96), (140, 28)], 168), (3, [(0, 64)], 64)):
        for calls in ([(31, 7)], [(13, 0), (6, 0)]):
            plain = dry(256, ny, bounds, transport, dict(options), calls, precision, dump=1)
            sponge = dry(256, ny, bounds, transport, dict(options, sponge=48), calls, precision, dump=1)
            assert plain[0] == 0 and sponge == plain and len(plain[1]) > 100
    rc, text = dry(256, 64, [(0, 64)], 3, dict(options, sponge=256), [(6, 0)], precision)
    assert rc < 0 and text == "lbm_set_sponge: width = 256 (0 .. nx - 1 = 255 only: column 0 keeps tau)"


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_help_names_the_sponge(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "[--sponge WIDTH:TAU_END]" in pr.stdout and "--sponge WIDTH:TAU_END: outlet sponge zone" in pr.stdout


def refused(solver, tmp_path, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("--sponge"), pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)
    return lines[0]


@pytest.mark.parametrize("value, why", [("abc", "is not a pair WIDTH:TAU_END"), ("48", "is not a pair WIDTH:TAU_END"), ("48:1.5:3", "is not a pair WIDTH:TAU_END"),
                                        ("", "is not a pair WIDTH:TAU_END"), (":", "has no whole number WIDTH"), ("48:", "has no number TAU_END"),
                                        (":1.5", "has no whole number WIDTH"), ("48x:1.5", "has no whole number WIDTH"), ("4.5:1.5", "has no whole number WIDTH"),
                                        ("48:1.5 ", "has no number TAU_END"), (" 48:1.5", "has no whole number WIDTH"), ("48:nan", "not a finite number above 0.5"),
                                        ("48:inf", "not a finite number above 0.5"), ("48:0.5", "not a finite number above 0.5"),
                                        ("-1:1.5", "width below 0")])
def test_malformed_pair_exits_2_before_a_device_opens(solver, tmp_path, value, why):
    line = refused(solver, tmp_path, ["--sponge", value])
    assert why in line and "'%s'" % value in line, line


def test_sponge_needs_a_width_the_grid_holds_and_tau_above_one_half(solver, tmp_path):
    assert refused(solver, tmp_path, ["--nx", "64", "--ny", "64", "--sponge", "64:1.5"]) == \
        "--sponge: width = 64 (0 .. nx - 1 = 63 only: column 0 keeps tau)"
    assert refused(solver, tmp_path, ["--tau", "0.5", "--nx", "64", "--ny", "64", "--sponge", "48:1.5"]) == \
        "--sponge: tau = 0.5 (the sponge's rates need tau > 0.5)"


@pytest.mark.parametrize("other, which, v1, v2", [(["--smagorinsky", "0.17"], LES, 0.17, 0.0), (["--trt-magic", "0.25"], TRT, 0.25, 0.0),
                                                  (["--forcing", "2e-5,-1e-5"], FORCING, 2e-5, -1e-5), (["--mrt", "1.0,0.1875"], MRT, 1.0, 0.1875)])
def test_sponge_with_another_collision_exits_2_with_the_librarys_text(lbm, solver, tmp_path, other, which, v1, v2):
    out, _ = setters(lbm, [(which, v1, v2), (SPONGE, 48, 1.5)])
    library = out[1][1]
    assert library.startswith("lbm_set_sponge: ") and "cannot be combined" in library
    for args in (other + ["--sponge", "48:1.5"], ["--sponge", "48:1.5"] + other):
        assert refused(solver, tmp_path, ["--nx", "64", "--ny", "64"] + args) == "--sponge: " + library[len("lbm_set_sponge: "):]


# ---- 8. the sponge lowers what comes back from the outlet ---------------------------------------------------------------------------------
def test_sponge_lowers_what_the_outlet_sends_back():
    """200x40, tau 0.53, u 0.08, disc r 0.1, W = 48, tau_end = 1.5, 700 iterations (tests/sponge_reference.py reflection_pair): the largest
    |rho - mean| over columns 60..119, upstream of the zone, once the start-up wave has met the outlet and come back. On the reference
    alone; the two values are written in profiles/sponge/README.md."""
    plain, sponge = reflection_pair()
    record("sponge_reflection", nx=R_NX, ny=R_NY, width=R_W, tau_end=R_TAU_END, steps=R_STEPS, plain=plain, sponge=sponge)
    print("largest |rho - mean| over columns 60..119 after %d iterations: plain BGK %.4g, sponge %.4g" % (R_STEPS, plain, sponge))
    assert sponge < plain, (sponge, plain)
