"""The MRT collision (lbm_set_mrt), the parts that need no GPU: the numpy reference operator of tests/mrt_reference.py against the
textbook moment-space form and its special cases, so that the GPU parity of tests/test_gpu_mrt.py means something; the setters and
their refusals through the library's device-less hook; checkpoint heads; the plan candidates; lbm_solver's --mrt."""
import ctypes
import functools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import PKG, lbm_cpu, record, solver  # noqa: F401
from tests.mrt_reference import BULK, MAGIC, mrt_cells, mrt_collide, mrt_rates, reference
from tests.reference import CX, CY, feq, oracle_run, trt_collide
from tests.test_ckpt_cpu import ALL, MASK_D, PROFILE_D, SCHED_D, WALLS, describe, head, pack  # noqa: F401
from tests.test_trt_cpu import candidates

MRT_BASE, MRT_BIT = 16, 1024


# ---- 1. the reference against the textbook form ---------------------------------------------------------------------------------------
def lallemand_luo():
    """The 9 x 9 moment matrix of Lallemand and Luo (2000) for the numbering of tests/reference.py, rows rho, e, eps, jx, qx, jy, qy,
    pxx, pxy."""
    cx, cy = np.array(CX, dtype=np.float64), np.array(CY, dtype=np.float64)
    c2 = cx * cx + cy * cy
    return np.array([np.ones(9), -4.0 + 3.0 * c2, 4.0 - 10.5 * c2 + 4.5 * c2 * c2, cx, (-5.0 + 3.0 * c2) * cx, cy, (-5.0 + 3.0 * c2) * cy,
                     cx * cx - cy * cy, cx * cy])


def test_moment_matrix_is_the_textbook_one():
    M = lallemand_luo()
    assert M[1].tolist() == [-4, -1, -1, -1, -1, 2, 2, 2, 2] and M[2].tolist() == [4, -2, -2, -2, -2, 1, 1, 1, 1]
    assert M[4].tolist() == [0, -2, 0, 2, 0, 1, -1, -1, 1] and M[6].tolist() == [0, 0, -2, 0, 2, 1, 1, -1, -1]
    assert M[7].tolist() == [0, 1, -1, 1, -1, 0, 0, 0, 0] and M[8].tolist() == [0, 0, 0, 0, 0, 1, -1, 1, -1]
    G = M @ M.T
    assert np.array_equal(G, np.diag(np.diag(G)))           # the rows are orthogonal


@pytest.mark.parametrize("tau, bulk, magic", [(0.55, 1.0, 3.0 / 16.0), (0.8, 0.3, 0.25), (1.3, 1.9, 0.01), (0.51, 1.0 / 0.51, 1.0)])
def test_reference_is_the_moment_space_operator(tau, bulk, magic):
    rng = np.random.default_rng(7)
    n = 4096
    r0 = 1.0 + 0.05 * (rng.random(n) - 0.5)
    u0, v0 = 0.2 * (rng.random(n) - 0.5), 0.2 * (rng.random(n) - 0.5)
    f = [feq(i, r0, u0, v0, u0 * u0 + v0 * v0) * (1.0 + 1e-2 * (rng.random(n) - 0.5)) for i in range(9)]
    assert all(np.all(x > 0.0) for x in f)
    r = np.zeros(n); jx = np.zeros(n); jy = np.zeros(n)
    for i in range(9):
        r = r + f[i]; jx = jx + float(CX[i]) * f[i]; jy = jy + float(CY[i]) * f[i]
    vx, vy = jx / r, jy / r
    out = np.array(mrt_cells(f, r, vx, vy, tau, bulk, magic))
    sb, wp, wm = mrt_rates(tau, bulk, magic)
    M, S = lallemand_luo(), np.diag([0.0, sb, sb, 0.0, wm, 0.0, wm, wp, wp])
    F = np.array(f)
    FE = np.array([feq(i, r, vx, vy, vx * vx + vy * vy) for i in range(9)])
    want = F - np.linalg.solve(M, S @ (M @ (F - FE)))
    scale = float(np.max(np.abs(F)))
    err = float(np.max(np.abs(out - want))) / scale
    mass = float(np.max(np.abs(out.sum(axis=0) - F.sum(axis=0)))) / scale
    mx = float(np.max(np.abs(sum(float(CX[i]) * (out[i] - F[i]) for i in range(9))))) / scale
    my = float(np.max(np.abs(sum(float(CY[i]) * (out[i] - F[i]) for i in range(9))))) / scale
    record("mrt_reference_vs_moment_space", tau=tau, bulk=bulk, magic=magic, err=err, mass=mass, mx=mx, my=my)
    assert err <= 1e-13, err
    assert mass <= 1e-13 and mx <= 1e-13 and my <= 1e-13, (mass, mx, my)


# ---- 2. special cases ---------------------------------------------------------------------------------------------------------------
def test_bulk_rate_one_over_tau_is_trt_and_degenerate_magic_is_bgk():
    nx, ny, steps = 200, 64, 97
    kw = dict(tau=0.55, inlet_velocity=0.06)
    tau = kw["tau"]
    mrt = oracle_run(nx, ny, steps, 0, collide=functools.partial(mrt_collide, bulk_rate=1.0 / tau, magic=MAGIC), **kw).f_next
    trt = oracle_run(nx, ny, steps, 0, collide=functools.partial(trt_collide, magic=MAGIC), **kw).f_next
    vs_trt = float(np.max(np.abs(mrt - trt))) / float(np.max(np.abs(trt)))
    magic = (tau - 0.5) ** 2
    deg = oracle_run(nx, ny, steps, 0, collide=functools.partial(mrt_collide, bulk_rate=1.0 / tau, magic=magic), **kw).f_next
    bgk = oracle_run(nx, ny, steps, 0, **kw).f_next
    vs_bgk = float(np.max(np.abs(deg - bgk))) / float(np.max(np.abs(bgk)))
    record("mrt_special_cases", vs_trt_rel=vs_trt, vs_bgk_rel=vs_bgk)
    assert vs_trt <= 1e-10, vs_trt
    assert vs_bgk <= 1e-10, vs_bgk


# ---- 3. the operator is active --------------------------------------------------------------------------------------------------------
def test_operator_is_active_and_stable_on_the_disc_case():
    ref, away = reference("disc")
    record("mrt_away_from_trt", max_abs=away)
    assert ref.first_unstable == -1
    assert away > 1e-6, away


# ---- 4. setters and refusals, without a device ------------------------------------------------------------------------------------------
LES, TRT, FORCING, MRT, INITIALISED, INITIALISE_DEEP = range(6)


def setters(lbm, calls, tau=0.55, precision=0, options=""):
    """lbm_debug_collision_setters: calls = [(setter, v1, v2)]. Returns ([(rc, text)], (collision, bulk rate, magic))."""
    L = lbm.lib()
    fn = L.lbm_debug_collision_setters
    fn.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double),
                   ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_double)]
    n = len(calls)
    which = (ctypes.c_int * n)(*[c[0] for c in calls])
    v1 = (ctypes.c_double * n)(*[c[1] for c in calls])
    v2 = (ctypes.c_double * n)(*[c[2] for c in calls])
    rc = (ctypes.c_int * n)()
    buf = ctypes.create_string_buffer(1 << 14)
    state = (ctypes.c_double * 3)()
    got = fn(tau, precision, options.encode(), which, v1, v2, n, rc, buf, len(buf), state)
    assert got == 0, L.lbm_last_error()
    lines = buf.value.decode().split("\n")[:n]
    return list(zip(list(rc), lines)), (int(state[0]), state[1], state[2])


def test_library_exports_the_two_symbols(lbm):
    L = lbm.lib()
    assert L.lbm_set_mrt.argtypes == [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    sb, magic = ctypes.c_double(), ctypes.c_double()
    assert L.lbm_set_mrt(None, 1.0, 0.25) == -1 and b"lbm_set_mrt: null context" in L.lbm_last_error()
    assert L.lbm_get_mrt(None, ctypes.byref(sb), ctypes.byref(magic)) == -1 and b"lbm_get_mrt: null context" in L.lbm_last_error()


def test_set_and_get(lbm):
    out, state = setters(lbm, [(MRT, 1.0, 0.1875)])
    assert out == [(0, "")] and state == (MRT_BASE, 1.0, 0.1875)
    for sb, magic in ((1e-300, 1.0), (1.9999999, 1e-300), (1.0 / 0.55, 0.25)):
        out, state = setters(lbm, [(MRT, sb, magic)])
        assert out == [(0, "")] and state == (MRT_BASE, sb, magic)
    # bulk_rate == 0 clears the model, whatever the (finite) magic parameter; on a context without it nothing changes
    for calls in ([(MRT, 1.0, 0.25), (MRT, 0.0, 0.25)], [(MRT, 0.0, 0.0)], [(MRT, 0.0, -3.0)], [(MRT, 1.0, 0.25), (MRT, 0.0, 7.0)]):
        out, state = setters(lbm, calls)
        assert all(rc == 0 for rc, _ in out) and state == (0, 0.0, 0.0), (calls, out, state)
    out, state = setters(lbm, [(TRT, 0.25, 0.0), (MRT, 0.0, 0.0)])            # clearing MRT leaves another model alone
    assert out == [(0, ""), (0, "")] and state[0] == 4


@pytest.mark.parametrize("sb, magic, text", [
    (float("nan"), 0.25, "lbm_set_mrt: bulk rate = nan (0, or finite values in (0, 2) only)"),
    (float("inf"), 0.25, "lbm_set_mrt: bulk rate = inf (0, or finite values in (0, 2) only)"),
    (-0.5, 0.25, "lbm_set_mrt: bulk rate = -0.5 (0, or finite values in (0, 2) only)"),
    (2.0, 0.25, "lbm_set_mrt: bulk rate = 2 (0, or finite values in (0, 2) only)"),
    (1.0, float("nan"), "lbm_set_mrt: magic parameter = nan (finite values only)"),
    (0.0, float("inf"), "lbm_set_mrt: magic parameter = inf (finite values only)"),
    (1.0, 0.0, "lbm_set_mrt: magic parameter = 0 (finite values in (0, 1] only)"),
    (1.0, -0.25, "lbm_set_mrt: magic parameter = -0.25 (finite values in (0, 1] only)"),
    (1.0, 1.5, "lbm_set_mrt: magic parameter = 1.5 (finite values in (0, 1] only)"),
])
def test_bad_values_are_refused_by_name(lbm, sb, magic, text):
    out, state = setters(lbm, [(MRT, sb, magic)])
    assert out == [(-1, text)] and state == (0, 0.0, 0.0)


def test_tau_and_initialised_context_are_refused(lbm):
    for tau in (0.5, 0.3):
        out, state = setters(lbm, [(MRT, 1.0, 0.25)], tau=tau)
        assert out == [(-1, "lbm_set_mrt: tau = %g (the MRT rates need tau > 0.5)" % tau)] and state[0] == 0
        assert setters(lbm, [(MRT, 0.0, 0.25)], tau=tau)[0] == [(0, "")]
    out, state = setters(lbm, [(MRT, 1.0, 0.25), (INITIALISED, 0, 0), (MRT, 0.5, 0.25), (MRT, 0.0, 0.0)])
    assert out[2] == out[3] == (-1, "lbm_set_mrt must be called before lbm_initialise") and state == (MRT_BASE, 1.0, 0.25)


OTHERS = [(LES, 0.17, 0.0, "lbm_set_smagorinsky: Cs = 0.17", "Smagorinsky constant Cs = 0.17"),
          (TRT, 0.25, 0.0, "lbm_set_trt: magic parameter 0.25", "TRT magic parameter 0.25"),
          (FORCING, 2e-5, -1e-5, "lbm_set_forcing: force (2e-05, -1e-05)", "forcing F = (2e-05, -1e-05)")]
MRT_HAS = "MRT parameters (bulk rate, magic) = (1, 0.1875)"


@pytest.mark.parametrize("which, v1, v2, sets, has", OTHERS)
def test_mutual_exclusion_in_both_orders(lbm, which, v1, v2, sets, has):
    out, state = setters(lbm, [(which, v1, v2), (MRT, 1.0, 0.1875)])
    assert out[0] == (0, "") and state[0] == (2, 4, 8)[which]
    assert out[1] == (-1, "lbm_set_mrt: (bulk rate, magic) = (1, 0.1875) on a context with %s (the two collisions cannot be combined)" % has)
    out, state = setters(lbm, [(MRT, 1.0, 0.1875), (which, v1, v2)])
    assert out[0] == (0, "") and state == (MRT_BASE, 1.0, 0.1875)
    assert out[1] == (-1, "%s on a context with %s (the two collisions cannot be combined)" % (sets, MRT_HAS))
    # either model cleared, the other is taken
    out, state = setters(lbm, [(MRT, 1.0, 0.1875), (MRT, 0.0, 0.0), (which, v1, v2)])
    assert [rc for rc, _ in out] == [0, 0, 0] and state[0] == (2, 4, 8)[which]
    out, state = setters(lbm, [(which, v1, v2), (which, 0.0, 0.0), (MRT, 1.0, 0.1875)])
    assert [rc for rc, _ in out] == [0, 0, 0] and state == (MRT_BASE, 1.0, 0.1875)


# ---- the table's row: plan candidates, kernel names, the shapes withheld ----------------------------------------------------------------
def mrt_row(lbm):
    """(tall, park) of the MRT row of collision_models, as the plan candidates of a large grid show them."""
    tall = any("deep=8" in c[1] for c in candidates(lbm, 1, MRT_BASE + 1))
    park = any(re.search(r"deep=1[01]\b", c[1]) for c in candidates(lbm, 0, MRT_BASE + 1))
    return tall, park


def test_mrt_kernels_ride_in_trts_objects(lbm):
    """The build list holds the models that have objects of their own; MRT shares TRT's pair code and is instantiated in TRT's objects
    (collision_models: unit). The library then defines the MRT launchers of every family (the register kernel's on the 64x32 regions,
    kind 0, alone: park and tall are false), and leaves none unresolved (tests/test_collision_units_cpu.py)."""
    build = __import__(PKG + ".build", fromlist=["build"])
    assert MRT_BASE not in build.COLLISION_BASES and 4 in build.COLLISION_BASES
    units = build.units("0123456789abcdef")
    assert not [obj for _, flags, obj in units if any(f.endswith("=%d" % MRT_BASE) for f in flags)]
    tall, park = mrt_row(lbm)
    assert not tall and not park
    out = subprocess.run(["nm", "-D", "--defined-only", "--demangle", build.build_all()], stdout=subprocess.PIPE, text=True, check=True,
                         timeout=60).stdout
    for t in ("double", "float"):
        for launcher in ("launch_site<%s, 16>", "launch_deep<%s, 16>", "launch_tile<%s, 16>", "launch_col<%s, 0, 16>", "launch_col<%s, 0, 17>"):
            assert "lbmk::" + launcher % t + "(" in out, launcher % t
    assert "launch_col<double, 2, 17>" not in out and "launch_col<float, 1, 1" + "7>" not in out and "launch_col<float, 1, 16>" not in out


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("arith", [0, 1])
def test_mrt_plan_candidates_and_kernel_names(lbm, precision, arith):
    tall, park = mrt_row(lbm)
    bgk = candidates(lbm, precision, arith)
    mrt = candidates(lbm, precision, arith + MRT_BASE)

    def keep(c):
        return ("deep=8" not in c[1] or tall) and (not re.search(r"deep=1[01]\b", c[1]) or park)
    assert mrt and all(c[2].endswith(",%d>" % (arith + MRT_BASE)) for c in mrt)
    assert [c for c in bgk if keep(c)] == [c[:2] + [c[2][:-len("%d>" % (arith + MRT_BASE))] + "%d>" % arith] + c[3:] for c in mrt]


def test_withheld_shapes_are_refused_with_the_tables_text(lbm):
    tall, park = mrt_row(lbm)
    noun = r"multiple-relaxation-time (MRT)"
    if not tall:          # the fp32 64x48 regions: BGK's alone
        out, state = setters(lbm, [(MRT, 1.0, 0.25)], precision=1, options="tune=0 deep=8")
        assert out == [(-1, "deep 8 (64x48 regions in registers) has no %s kernel" % noun)] and state[0] == 0
    for deep in (10, 11):
        out, state = setters(lbm, [(MRT, 1.0, 0.25), (INITIALISE_DEEP, 0, 0)], options="tune=0 arith=1 deep=%d" % deep)
        if park:
            assert out == [(0, ""), (0, "")]
        else:
            assert out == [(-1, "deep %d (64x40 regions in registers) has no %s kernel" % (deep, noun)), (0, "")] and state[0] == 0
    for deep in (6, 7, 9):      # the 64x32 regions every model has
        assert setters(lbm, [(MRT, 1.0, 0.25), (INITIALISE_DEEP, 0, 0)], options="tune=0 arith=1 deep=%d" % deep)[0] == [(0, ""), (0, "")]


# ---- checkpoint heads ---------------------------------------------------------------------------------------------------------------------
PAIR = (BULK, MAGIC)
PORTS = (1.0, 1.004, 1.0, 0.996)


def mrt_head(lbm, params=PAIR, ports=False, periodic=False, **fields):
    d = describe(**fields)
    h = lbm.CkptHead(**d.fixed)
    h.has_mask, h.mask_digest = d.mask is not None, d.mask or 0
    h.has_profile, h.profile_digest = d.profile is not None, d.profile or 0
    h.has_sched, h.sched_digest = d.sched is not None, d.sched or 0
    if d.walls is not None:
        h.has_walls, h.walls = 1, (ctypes.c_double * 4)(*d.walls)
    if params is not None:
        h.collision, h.collision_param = MRT_BASE, (ctypes.c_double * 2)(*params)
    if ports:
        h.has_ports, h.ports = 1, (ctypes.c_double * 4)(*PORTS)
    h.has_periodic_y = 1 if periodic else 0
    return h


def test_checkpoint_head_carries_the_pair_behind_ports_and_periodic_y(lbm):
    assert lbm.binding.CKPT_HEAD_MAX == 184
    data = lbm.debug_ckpt_save(mrt_head(lbm))
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Qdd", data[72:96]) == (MRT_BIT,) + PAIR and len(data) == 96
    data = lbm.debug_ckpt_save(mrt_head(lbm, ports=True, periodic=True))
    assert struct.unpack("<Q4ddd", data[72:128]) == (256 | 512 | MRT_BIT,) + PORTS + PAIR and len(data) == 128
    full = mrt_head(lbm, ports=True, periodic=True, mask=True, profile=True, walls=True, sched=True)
    data = lbm.debug_ckpt_save(full)
    assert len(data) == 184
    assert struct.unpack("<QQQ4dQ4ddd", data[72:184]) == (1 | 2 | 16 | 32 | 256 | 512 | MRT_BIT, MASK_D, PROFILE_D) + WALLS + (SCHED_D,) + PORTS + PAIR
    assert lbm.debug_ckpt_load(data, full) == 184 and lbm.debug_ckpt_load(data + bytes(100), full) == 184


def test_checkpoint_loads_only_into_equal_parameters(lbm):
    data = lbm.debug_ckpt_save(mrt_head(lbm))
    assert lbm.debug_ckpt_load(data, mrt_head(lbm)) == len(data)
    for other in ((0.9, MAGIC), (BULK, 0.25)):
        with pytest.raises(lbm.LbmError, match=r"written with MRT parameters \(bulk rate, magic\) = \(1, 0\.1875\); this context has \(bulk rate, magic\) = \(%s, %s\)"
                           % tuple(re.escape("%.17g" % v) for v in other)):
            lbm.debug_ckpt_load(data, mrt_head(lbm, params=other))
    # a file without the bit is refused by an MRT context, and the reverse
    bgk = lbm.debug_ckpt_save(mrt_head(lbm, params=None))
    assert bgk[:8] == b"LBMCKPT1"
    with pytest.raises(lbm.LbmError, match=r"written without a MRT parameters; this context has \(bulk rate, magic\) = \(1, 0\.1875\)"):
        lbm.debug_ckpt_load(bgk, mrt_head(lbm))
    with pytest.raises(lbm.LbmError, match=r"written with MRT parameters \(bulk rate, magic\) = \(1, 0\.1875\); this context has none"):
        lbm.debug_ckpt_load(data, mrt_head(lbm, params=None))
    # a TRT file into an MRT context and the reverse: MRT, the last row of the table, is named first
    trt = lbm.CkptHead(**describe().fixed)
    trt.collision, trt.collision_param = 4, (ctypes.c_double * 2)(MAGIC, 0.0)
    trt_bytes = lbm.debug_ckpt_save(trt)
    with pytest.raises(lbm.LbmError, match="written without a MRT parameters"):
        lbm.debug_ckpt_load(trt_bytes, mrt_head(lbm))
    with pytest.raises(lbm.LbmError, match="written with MRT parameters"):
        lbm.debug_ckpt_load(data, trt)
    # a head that announces two collision models is no checkpoint
    two = data[:72] + struct.pack("<Qddd", 8 | MRT_BIT, MAGIC, *PAIR)
    with pytest.raises(lbm.LbmError):
        lbm.debug_ckpt_load(two, mrt_head(lbm))


def test_the_64_earlier_descriptions_serialise_as_before(lbm, head):
    assert len(ALL) == 64
    for d in ALL:
        assert lbm.debug_ckpt_save(head(d)) == pack(d), d
        assert lbm.debug_ckpt_load(pack(d), head(d)) == len(pack(d)), d


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------------
def test_help_names_mrt(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "[--mrt BULK,MAGIC]" in pr.stdout and "--mrt BULK,MAGIC: multiple-relaxation-time (MRT) collision" in pr.stdout


def refused(solver, tmp_path, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk"] + args, cwd=tmp_path, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("--mrt"), pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)
    return lines[0]


@pytest.mark.parametrize("value, why", [("abc", "is not a pair BULK,MAGIC"), ("1.0", "is not a pair BULK,MAGIC"), ("1,0.25,3", "is not a pair BULK,MAGIC"),
                                        ("", "is not a pair BULK,MAGIC"), (",", "has no number BULK"), ("1.0,", "has no number MAGIC"),
                                        (",0.25", "has no number BULK"), ("1x,0.25", "has no number BULK"), ("1,0.25 ", "has no number MAGIC"),
                                        (" 1,0.25", "has no number BULK"), ("nan,0.25", "not finite"), ("1,inf", "not finite"),
                                        ("2,0.25", "bulk rate outside (0, 2)"), ("-1,0.25", "bulk rate outside (0, 2)"),
                                        ("1,0", "magic parameter outside (0, 1]"), ("1,1.5", "magic parameter outside (0, 1]")])
def test_malformed_pair_exits_2_before_a_device_opens(solver, tmp_path, value, why):
    line = refused(solver, tmp_path, ["--mrt", value])
    assert why in line and "'%s'" % value in line, line


def test_mrt_needs_tau_above_one_half(solver, tmp_path):
    assert refused(solver, tmp_path, ["--tau", "0.5", "--mrt", "1.0,0.25"]) == "--mrt: tau = 0.5 (the MRT rates need tau > 0.5)"


@pytest.mark.parametrize("other, which, v1, v2", [(["--smagorinsky", "0.17"], LES, 0.17, 0.0), (["--trt-magic", "0.25"], TRT, 0.25, 0.0),
                                                  (["--forcing", "2e-5,-1e-5"], FORCING, 2e-5, -1e-5)])
def test_mrt_with_another_collision_exits_2_with_the_librarys_text(lbm, solver, tmp_path, other, which, v1, v2):
    out, _ = setters(lbm, [(which, v1, v2), (MRT, 1.0, 0.1875)])
    library = out[1][1]
    assert library.startswith("lbm_set_mrt: ") and "cannot be combined" in library
    for args in (other + ["--mrt", "1.0,0.1875"], ["--mrt", "1.0,0.1875"] + other):
        assert refused(solver, tmp_path, args) == "--mrt: " + library[len("lbm_set_mrt: "):]
