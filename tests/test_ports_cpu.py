"""The two ports (lbm_set_port: pressure and velocity ports at the inlet and the outlet) without a GPU: the reference of
tests/ports_reference.py against the unmodified oracle loop, the kernels' port rule (lbm_debug_port_rule: the very inline function,
compiled for the host) against the numpy rule, the argument errors, the checkpoint head's row, lbm_solver's options, and the physics of
the reference on a pressure-driven channel, so that the GPU parity of tests/test_gpu_ports.py means something."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import test_ckpt_cpu as tc
from tests.helpers import lbm_cpu, solver  # noqa: F401
from tests.ports_reference import CHANNEL, DEFAULT_PORTS, PRESSURE, VELOCITY, channel_run, port_rule, ports_run
from tests.reference import FREESLIP, HOLD, NOSLIP, REPEAT, moving, oracle_run


# ---- the reference with default ports is the oracle loop --------------------------------------------------------------------------
@pytest.mark.parametrize("nx, ny, steps, kw", [
    (60, 24, 40, dict(walls=(FREESLIP, moving(0.05)), schedule=(np.linspace(0.2, 1.0, 7), HOLD), tau=0.6, inlet_velocity=0.05, cylinder_radius=0.15)),
    (33, 17, 25, dict(walls=(moving(-0.03), NOSLIP), schedule=(np.array([1.0, 0.5, 0.75]), REPEAT), tau=0.8, inlet_velocity=0.03, cylinder_radius=0.1)),
    (1, 9, 6, dict(walls=NOSLIP, tau=0.7, inlet_velocity=0.02, cylinder_radius=0.0)),
])
def test_default_ports_are_the_oracle_loop_bit_for_bit(nx, ny, steps, kw):
    want, want_cur = oracle_run(nx, ny, steps, 8, keep_f_current=True, **kw)
    for ports in (DEFAULT_PORTS, (None, None), (VELOCITY, (PRESSURE, 1.0))):
        got, got_cur = ports_run(nx, ny, steps, 8, ports=ports, keep_f_current=True, **kw)
        for a, b in zip(got[:4] + (got_cur,), want[:4] + (want_cur,)):
            assert np.array_equal(a, b)
        assert got.forces == want.forces and got.first_unstable == want.first_unstable == -1 and got.solid_count == want.solid_count


@pytest.mark.parametrize("ports", [(VELOCITY, (PRESSURE, 0.985)), ((PRESSURE, 1.02), (PRESSURE, 1.0)), ((PRESSURE, 1.015), (VELOCITY, 0.03)),
                                   (VELOCITY, (VELOCITY, 0.04))])
def test_every_port_pair_changes_the_populations_and_stays_stable(ports):
    kw = dict(walls=(FREESLIP, moving(0.05)), tau=0.6, inlet_velocity=0.05, cylinder_radius=0.15)
    base = oracle_run(60, 24, 40, 0, **kw)
    run = ports_run(60, 24, 40, 0, ports=ports, **kw)
    assert run.first_unstable == -1 and not np.array_equal(run.f_next, base.f_next)
    west, east = ports
    if west != VELOCITY:
        assert np.all(run.rho[:, 0] == west[1])
    if east[0] == PRESSURE:
        assert np.all(run.rho[:, -1] == east[1])
    else:
        assert np.all(run.ux[:, -1] == east[1])


# ---- the kernels' rule on one cell ---------------------------------------------------------------------------------------------------
CASES = [("west", VELOCITY, 0.0), ("west", PRESSURE, 1.013), ("east", PRESSURE, 0.991), ("east", VELOCITY, 0.037)]


def cells(n, seed):
    rng = np.random.default_rng(seed)
    w = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4)
    return w[None, :] * (1.0 + 0.2 * (rng.random((n, 9)) - 0.5))


@pytest.mark.parametrize("precision, dtype", [("f64", np.float64), ("f32", np.float32)])
@pytest.mark.parametrize("side, kind, value", CASES)
def test_debug_port_rule_is_the_numpy_rule_bit_for_bit(lbm, side, kind, value, precision, dtype):
    f = cells(200, 11)
    u_in = np.random.default_rng(12).uniform(-0.1, 0.1, len(f))
    for k in range(len(f)):
        got, rho, u = lbm.debug_port_rule(side, kind, value, f[k], u_in=u_in[k], precision=precision)
        want = f[k:k + 1].astype(dtype)
        given = dtype(u_in[k]) if (side, kind) == ("west", VELOCITY) else dtype(value)
        wr, wu = port_rule(want, 0 if side == "west" else 1, kind, given)
        assert want.dtype == dtype and wr.dtype == dtype and wu.dtype == dtype
        assert np.array_equal(got, want[0].astype(np.float64)), (k, got, want)
        assert rho == float(wr[0]) and u == float(wu[0])
        # the given one comes back as cast
        assert (u if kind == VELOCITY else rho) == float(given)


@pytest.mark.parametrize("precision, T", [("f64", np.float64), ("f32", np.float32)])
def test_default_ports_are_the_expressions_of_the_reference(lbm, precision, T):
    """The velocity inlet and the rho = 1 outlet as they were written before the ports (LBMSolver.h:181-235), in the element type."""
    for f64 in cells(100, 13):
        f = f64.astype(T)
        u_in = T(0.0421)
        rho_bc = (f[0] + f[2] + f[4] + T(2.0) * (f[3] + f[6] + f[7])) / (T(1.0) - u_in)
        want = f.copy()
        want[1] = f[3] + T(2.0 / 3.0) * rho_bc * u_in
        want[5] = f[7] - T(0.5) * (f[2] - f[4]) + T(1.0 / 6.0) * rho_bc * u_in
        want[8] = f[6] + T(0.5) * (f[2] - f[4]) + T(1.0 / 6.0) * rho_bc * u_in
        got, rho, u = lbm.debug_port_rule("west", VELOCITY, 0.0, f64, u_in=0.0421, precision=precision)
        assert np.array_equal(got, want.astype(np.float64)) and rho == float(rho_bc) and u == float(u_in)
        u_out = T(-1.0) + (f[0] + f[2] + f[4] + T(2.0) * (f[1] + f[5] + f[8]))
        want = f.copy()
        want[3] = f[1] - T(2.0 / 3.0) * u_out
        want[6] = f[8] - T(0.5) * (f[2] - f[4]) - T(1.0 / 6.0) * u_out
        want[7] = f[5] + T(0.5) * (f[2] - f[4]) - T(1.0 / 6.0) * u_out
        got, rho, u = lbm.debug_port_rule("east", PRESSURE, 1.0, f64, precision=precision)
        assert np.array_equal(got, want.astype(np.float64)) and rho == 1.0 and u == float(u_out)


# ---- the argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_offender(lbm):
    L = lbm.lib()
    k, v = C.c_int(), C.c_double()
    assert L.lbm_set_port(None, 0, 1, 1.01) == -1 and b"lbm_set_port: null context" in L.lbm_last_error()
    assert L.lbm_get_port(None, 0, C.byref(k), C.byref(v)) == -1 and b"lbm_get_port: null context" in L.lbm_last_error()
    # the checks lbm_set_port shares with the hook (the GPU file runs them on a context)
    f = (C.c_double * 9)(*([0.1] * 9))
    out = (C.c_double * 9)()
    for side, kind, value, text in [(2, 1, 1.0, b"side = 2"), (-1, 1, 1.0, b"side = -1"), (0, 2, 1.0, b"kind = 2"), (1, -1, 1.0, b"kind = -1"),
                                    (0, 1, float("nan"), b"value = nan"), (1, 0, float("inf"), b"value = inf"), (0, 1, 0.0, b"pressure = 0"),
                                    (1, 1, -0.5, b"pressure = -0.5"), (1, 0, 1.0, b"east velocity = 1"), (1, 0, -1.5, b"east velocity = -1.5"),
                                    (0, 0, 0.01, b"with a west velocity port")]:
        assert L.lbm_debug_port_rule(side, kind, value, 0.0, 0, f, out, None, None) == -1, (side, kind, value)
        assert text in L.lbm_last_error() and b"lbm_debug_port_rule" in L.lbm_last_error(), L.lbm_last_error()
    assert L.lbm_debug_port_rule(0, 0, 0.0, 0.0, 2, f, out, None, None) == -1 and b"precision" in L.lbm_last_error()
    assert L.lbm_debug_port_rule(0, 0, 0.0, 0.0, 0, None, out, None, None) == -1 and b"null" in L.lbm_last_error()
    assert L.lbm_debug_port_rule(0, 0, 0.0, 1.0, 0, f, out, None, None) == -1 and b"u_in" in L.lbm_last_error()
    assert L.lbm_debug_port_rule(1, 0, -0.999, 0.0, 1, f, out, None, None) == 0
    with pytest.raises(ValueError):
        lbm.debug_port_rule("north", PRESSURE, 1.0, [0.1] * 9)
    with pytest.raises(ValueError):
        lbm.debug_port_rule("east", "suction", 1.0, [0.1] * 9)
    # ports=: the bare name is the west velocity port alone
    assert lbm.binding._port_pair(("velocity", None)) == ((0, 0.0), (1, 1.0))
    assert lbm.binding._port_pair((("pressure", 1.01), ("velocity", 0.03))) == ((1, 1.01), (0, 0.03))
    for bad in ((None, "velocity"), ("pressure", None), (None, "pressure")):
        with pytest.raises(ValueError, match="place"):
            lbm.binding._port_pair(bad)


# ---- the checkpoint head ---------------------------------------------------------------------------------------------------------------
PORTS = (1.0, 1.01, 1.0, 0.99)                 # west kind, west value, east kind, east value


@pytest.fixture(scope="module")
def ported(lbm):
    """tests/test_ckpt_cpu.py's head of a description, with ports on top."""
    def make(d, ports=PORTS):
        h = lbm.CkptHead(**d.fixed)
        h.has_mask, h.mask_digest = d.mask is not None, d.mask or 0
        h.has_profile, h.profile_digest = d.profile is not None, d.profile or 0
        h.has_sched, h.sched_digest = d.sched is not None, d.sched or 0
        if d.collision:
            h.collision = tc.MODELS[d.collision][0]
            h.collision_param = (C.c_double * 2)(*d.params)
        if d.walls is not None:
            h.has_walls, h.walls = 1, (C.c_double * 4)(*d.walls)
        if ports is not None:
            h.has_ports, h.ports = 1, (C.c_double * 4)(*ports)
        return h
    return make


def packed(d, ports=PORTS):
    """tests/test_ckpt_cpu.py's documented bytes of a description, with flag 256 and the four doubles behind everything else."""
    data = tc.pack(d)
    if data[:8] != b"LBMCKPT3":
        flags, rest = (1, data[72:]) if data[:8] == b"LBMCKPT2" else (0, b"")
    else:
        flags, rest = struct.unpack("<Q", data[72:80])[0], data[80:]
    return b"LBMCKPT3" + data[8:72] + struct.pack("<Q", flags | 256) + rest + struct.pack("<4d", *ports)


def test_the_bytes_of_a_head_with_ports(lbm, ported):
    assert lbm.binding.CKPT_HEAD_MAX == 184
    for d in tc.ALL:
        assert lbm.debug_ckpt_save(ported(d, None)) == tc.pack(d), d            # has_ports = 0: the 64 descriptions as they were
        data = lbm.debug_ckpt_save(ported(d))
        assert data == packed(d) and len(data) <= lbm.binding.CKPT_HEAD_MAX, d
    data = lbm.debug_ckpt_save(ported(tc.describe()))
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q4d", data[72:112]) == (256,) + PORTS and len(data) == 112
    data = lbm.debug_ckpt_save(ported(tc.describe(sched=True)))              # behind a schedule's digest
    assert struct.unpack("<QQ4d", data[72:120]) == (32 | 256, tc.SCHED_D) + PORTS
    full = tc.describe(True, True, "forced", True, True)                     # the longest head
    assert len(lbm.debug_ckpt_save(ported(full))) == 184
    assert struct.unpack("<Q", lbm.debug_ckpt_save(ported(full))[72:80]) == (1 | 2 | 16 | 32 | 64 | 256,)


def test_heads_with_ports_load_into_equal_ports_only(lbm, ported):
    pre = "checkpoint x.ckpt was written "

    def refusal(data, here):
        try:
            assert lbm.debug_ckpt_load(data, here) == len(data)
        except lbm.LbmError as e:
            return str(e)
        return None
    for d in tc.ALL:
        assert refusal(packed(d), ported(d)) is None, d
        assert lbm.debug_ckpt_load(packed(d) + bytes(100), ported(d)) == len(packed(d))
        # without ports on either side every refusal is what it was
        for here in tc.ALL[::7]:
            want = tc.first_difference(d, here)
            msg = refusal(tc.pack(d), ported(here, None))
            assert (msg is None) == (want is None)
            if want:
                tc.check_refusal(msg, *want)
    none = tc.describe()
    other = (1.0, 1.01, 0.0, 0.03)
    assert refusal(packed(none), ported(none, None)) == pre + "with ports west kind 1 value 1.01, east kind 1 value 0.99; this context has the default ports"
    assert refusal(tc.pack(none), ported(none)) == pre + "with the default ports; this context has ports west kind 1 value 1.01, east kind 1 value 0.99"
    assert refusal(packed(none), ported(none, other)) == pre + ("with ports west kind 1 value 1.01, east kind 1 value 0.99; this context has "
                                                                "ports west kind 1 value 1.01, east kind 0 value 0.03")
    # the order: collision models, walls, then the ports, then profile, schedule, mask, header
    W, P = tc.describe(walls=True), tc.describe(profile=True)
    assert "wall" in refusal(packed(W), ported(none, None))
    assert "forcing" in refusal(packed(tc.describe(collision="forced")), ported(none, None))
    assert "ports" in refusal(packed(P), ported(none, None))
    assert "ports" in refusal(packed(tc.describe(True, True, None, False, True)), ported(none, None))
    assert refusal(packed(none), ported(none._replace(fixed=dict(tc.FIXED, tau=0.7)), other)).startswith(pre + "with ports")
    # truncated heads and the unassigned bit 7 are not checkpoints
    data = packed(none)
    for n in range(len(data)):
        assert refusal(data[:n], ported(none)) == "x.ckpt is not a checkpoint"
    assert refusal(data[:72] + struct.pack("<Q", 256 | 128) + data[80:] + bytes(64), ported(none)) == "x.ckpt is not a checkpoint"


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_help_documents_the_ports(solver):
    pr = subprocess.run([solver, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert pr.returncode == 0
    assert "[--inlet velocity|pressure:RHO] [--outlet pressure:RHO|velocity:U]" in pr.stdout
    assert "--inlet pressure:1.005 --outlet" in pr.stdout and "not constant along x" in pr.stdout and "do not know about --forcing" in pr.stdout


def refused(solver, tmp_path, args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    pr = subprocess.run([solver, "--steps", "1", "--no-vtk"] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                        text=True, timeout=60, env=env)
    assert pr.returncode == 2, (pr.stdout, pr.stderr)
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1, pr.stderr
    assert "MI355X HIP Grid" not in pr.stdout and not os.listdir(tmp_path)
    return lines[0]


@pytest.mark.parametrize("args, why", [
    (["--inlet", "pressure"], "is not a port kind"), (["--inlet", "velocity:0.1"], "is not a port kind"), (["--inlet", "pressure:"], "has no density"),
    (["--inlet", "pressure:1.0x"], "has no density"), (["--inlet", "pressure:0"], "not above 0"), (["--inlet", "pressure:-1"], "not above 0"),
    (["--inlet", "pressure:nan"], "not finite"), (["--outlet", "velocity"], "is not a port kind"), (["--outlet", "velocity:"], "has no velocity"),
    (["--outlet", "velocity:1"], "not below 1"), (["--outlet", "velocity:-inf"], "not finite"), (["--outlet", "pressure:0"], "not above 0"),
    (["--outlet", "suction:1"], "is not a port kind")])
def test_bad_ports_exit_2_before_a_device_opens(solver, tmp_path, args, why):
    line = refused(solver, tmp_path, args)
    assert line.startswith(args[0] + ": '" + args[1] + "'") and why in line, line


@pytest.mark.parametrize("other, name", [(["--inlet-profile", "parabolic"], "--inlet-profile"), (["--inlet-ramp", "20"], "--inlet-ramp"),
                                         (["--inlet-pulse", "0.1:16"], "--inlet-pulse")])
def test_a_pressure_inlet_takes_no_inlet_velocity(solver, tmp_path, other, name):
    for args in (["--inlet", "pressure:1.01"] + other, other + ["--inlet", "pressure:1.01"]):
        line = refused(solver, tmp_path, args)
        assert line.startswith("--inlet pressure:RHO cannot be combined with " + name), line


# ---- the physics of the reference: a channel driven by a density difference -------------------------------------------------------------
def test_pressure_driven_channel_of_the_reference():
    """All-fluid 48x17, tau = 1, from rest, ports (pressure 1.005, pressure 0.995), no-slip walls, 6000 iterations. Measured with this
    reference: steady to 4e-16 over 500 further iterations; the centreline velocity at x = nx / 2 is 0.9417 of G H^2 / (8 nu) with
    G = (rho_w - rho_e) / (3 (nx - 1)), H = ny - 1 (0.8908 at 32x13, tau 0.8); the mass flux is 0.242 at the inlet column, 0.137 at the
    mid column and 0.036 at the outlet column: the on-node walls exchange mass with the fluid wherever rho is not 1."""
    nx, ny, tau = CHANNEL["nx"], CHANNEL["ny"], CHANNEL["tau"]
    run, later = channel_run(6000), channel_run(6500)
    assert run.first_unstable == -1 and later.first_unstable == -1
    drift = float(np.max(np.abs(later.ux - run.ux)))
    mid = run.ux[:, nx // 2]
    G, H, nu = (1.005 - 0.995) / (3.0 * (nx - 1)), ny - 1, (tau - 0.5) / 3.0
    ratio = float(mid[ny // 2]) / (G * H * H / (8.0 * nu))
    flux = [float(np.sum(run.rho[:, x] * run.ux[:, x])) for x in (0, nx // 2, nx - 1)]
    print("channel: drift %.3g, ratio %.4f, mass flux inlet %.4f mid %.4f outlet %.4f" % ((drift, ratio) + tuple(flux)))
    assert drift < 1e-12
    assert np.all(mid[1:-1] > 0.0)
    assert float(np.max(np.abs(mid - mid[::-1]))) <= 1e-13          # symmetric about the centre row (the operations are not: round-off)
    assert 0.85 < ratio < 1.0
    assert np.all(run.rho[:, 0] == 1.005) and np.all(run.rho[:, -1] == 0.995)
