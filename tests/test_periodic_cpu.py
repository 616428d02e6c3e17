"""Periodic top and bottom boundaries (lbm_set_periodic_y) without a device: the reference of tests/periodic_reference.py (it is
oracle_run where periodic is off; roll invariance; every row differs from the walled run), the checkpoint head's bit 9, the dry runs of
the launch choreography of a lone periodic strip and of rings of strips on both transports, and the refusals that need no context
(the setter's null context, the dry-run hooks, lbm_solver's command line)."""
import ctypes as C
import importlib
import itertools
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import PKG, lbm_cpu, solver  # noqa: F401
from tests.periodic_reference import NX, NY, OF, STEPS, TAU, U0, periodic_run, seam_mask, seam_profile, seam_reference
from tests.reference import oracle_run
from tests.test_choreography_cpu import PLANS as CHOREO_PLANS
from tests.test_choreography_cpu import dry  # noqa: F401


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def test_the_reference_without_periodicity_is_oracle_run():
    kw = dict(mask=seam_mask(), u=seam_profile(), tau=TAU, inlet_velocity=U0)
    a = periodic_run(NX, NY, 25, OF, periodic=False, **kw)
    b = oracle_run(NX, NY, 25, OF, **kw)
    assert np.array_equal(a.f_next, b.f_next) and a.forces == b.forces
    for x, y in zip((a.rho, a.ux, a.uy), (b.rho, b.ux, b.uy)):
        assert np.array_equal(x, y)
    assert (a.first_unstable, a.solid_count) == (b.first_unstable, b.solid_count)
    walls = ("free-slip", ("moving", 0.03))
    a = periodic_run(64, 24, 12, 4, periodic=False, walls=walls, tau=0.7, inlet_velocity=0.04)
    b = oracle_run(64, 24, 12, 4, walls=walls, tau=0.7, inlet_velocity=0.04)
    assert np.array_equal(a.f_next, b.f_next) and a.forces == b.forces


@pytest.mark.parametrize("k", [1, 17, 36])
def test_roll_invariance_of_the_reference(k):
    """Rolling mask and profile by k rows rolls f_next by k rows, bit for bit (no row is special), and the forces with it."""
    a, b = seam_reference(), seam_reference(k)
    assert a.first_unstable == -1 and b.first_unstable == -1
    assert np.array_equal(np.roll(a.f_next[1:-1], k, axis=0), b.f_next[1:-1])
    for x, y in zip((a.rho, a.ux, a.uy), (b.rho, b.ux, b.uy)):
        assert np.array_equal(np.roll(x, k, axis=0), y)
    assert [r[0] for r in a.forces] == [r[0] for r in b.forces] == list(range(0, STEPS, OF))
    for (_, fx, fy), (_, gx, gy) in zip(a.forces, b.forces):        # (one sum over the cells in another order)
        assert abs(fx - gx) <= 1e-13 * max(1.0, abs(fx)) and abs(fy - gy) <= 1e-13 * max(1.0, abs(fy))


def test_the_walls_are_gone_and_a_uniform_stream_stays_uniform():
    per, walled = seam_reference(), seam_reference(periodic=False)
    assert np.all(np.any(per.f_next[1:-1, 1:-1] != walled.f_next[1:-1, 1:-1], axis=(1, 2)))       # every row differs from the walled run
    # the wrapped ghost rows are the opposite edge rows; the ghost columns stay zero, those of the wrapped rows included
    assert np.array_equal(per.f_next[0], per.f_next[-2]) and np.array_equal(per.f_next[-1], per.f_next[1])
    fluid = seam_reference(fluid=True)
    assert np.all(fluid.f_next[1:-1] == fluid.f_next[1:2])                                          # an all-fluid domain keeps all rows bit-equal
    fluid_walled = seam_reference(fluid=True, periodic=False)
    assert not np.all(fluid_walled.f_next[1:-1] == fluid_walled.f_next[1:2])


def test_forces_cross_the_seam():
    """A one-cell obstacle on row 0 feels the fluid of row ny - 1: its force is that of the same obstacle mid-channel, rolled there."""
    nx, ny = 64, 24
    m = np.zeros((ny, nx), np.uint8)
    m[0, 20] = 1
    a = periodic_run(nx, ny, 20, 5, mask=m, tau=0.6, inlet_velocity=0.05)
    b = periodic_run(nx, ny, 20, 5, mask=np.roll(m, 11, axis=0), tau=0.6, inlet_velocity=0.05)
    assert a.forces[-1][1] > 1e-4
    for (_, fx, fy), (_, gx, gy) in zip(a.forces, b.forces):
        assert abs(fx - gx) <= 1e-14 and abs(fy - gy) <= 1e-14


# ---- the checkpoint head -------------------------------------------------------------------------------------------------------------------
def head(lbm, **kw):
    h = lbm.CkptHead()
    h.nx, h.ny, h.y_start, h.local_ny, h.precision, h.steps_done = 200, 72, 0, 72, 0, 30
    h.tau, h.inlet_velocity, h.cylinder_x, h.cylinder_y, h.cylinder_radius = 0.6, 0.05, 0.2, 0.5, 0.05
    for k, v in kw.items():
        setattr(h, k, v)
    return h


def test_checkpoint_head_bit_9(lbm):
    per = head(lbm, has_periodic_y=1)
    data = lbm.debug_ckpt_save(per)
    assert data[:8] == b"LBMCKPT3" and len(data) == 80 and int.from_bytes(data[72:80], "little") == 512      # the flag is the field: no payload
    assert lbm.debug_ckpt_load(data, head(lbm, has_periodic_y=1)) == 80
    with pytest.raises(lbm.LbmError, match="checkpoint x.ckpt was written with periodic y; this context has two walls"):
        lbm.debug_ckpt_load(data, head(lbm))
    plain = lbm.debug_ckpt_save(head(lbm))
    assert plain[:8] == b"LBMCKPT1" and len(plain) == 72                                                       # without the call: what it was
    with pytest.raises(lbm.LbmError, match=r"was written without periodic y \(two walls\); this context has periodic y"):
        lbm.debug_ckpt_load(plain, head(lbm, has_periodic_y=1))
    # its rank: behind the walls, before the ports
    walls = head(lbm, has_walls=1, has_periodic_y=1)
    walls.walls[:] = [1.0, 0.0, 1.0, 0.0]
    with pytest.raises(lbm.LbmError, match="with wall kinds 1 .south. and 1 .north.; this context has two no-slip walls"):
        lbm.debug_ckpt_load(lbm.debug_ckpt_save(walls), head(lbm))
    ports = head(lbm, has_ports=1, has_periodic_y=1)
    ports.ports[:] = [1.0, 1.01, 1.0, 0.99]
    with pytest.raises(lbm.LbmError, match="was written with periodic y; this context has two walls"):
        lbm.debug_ckpt_load(lbm.debug_ckpt_save(ports), head(lbm))
    both = lbm.debug_ckpt_save(ports)
    assert int.from_bytes(both[72:80], "little") == 256 | 512 and len(both) == 80 + 32
    assert lbm.debug_ckpt_load(both, ports) == 112
    # bit 7 stays "not a checkpoint", with bit 9 beside it too
    for flags in (128, 128 | 512):
        bad = bytearray(data)
        bad[72:80] = flags.to_bytes(8, "little")
        with pytest.raises(lbm.LbmError, match="is not a checkpoint"):
            lbm.debug_ckpt_load(bytes(bad), per)
    assert importlib.import_module(PKG + ".binding").CKPT_HEAD_MAX == 184          # (LBM_CKPT_HEAD_MAX stays: bit 9 adds no byte)


# ---- the dry runs ----------------------------------------------------------------------------------------------------------------------------
STRIP_PLANS = CHOREO_PLANS          # (every plan of the choreography tests is one a strip may run; the fp64 64x40 regions, deep 10 / 11, are not among them)
GEOMETRIES = [([(0, 72)], 72), ([(0, 12)], 12), ([(0, 36), (36, 36)], 72), ([(0, 12), (12, 12)], 24), ([(0, 24), (24, 12), (36, 36)], 72),
              ([(0, 200), (200, 13), (213, 87)], 300)]
PERIODIC_CALLS = [[(13, 5), (1, 0), (20, 5)], [(60, 0)], [(7, 0), (97, 31)], [(2, 0)]]


def test_no_race_and_no_stale_row_on_the_ring(dry):  # noqa: F811
    runs = 0
    for (plan, prec), dh, ov in itertools.product(STRIP_PLANS, (0, 2), (0, 1, 2)):
        for (bounds, ny), transport, calls in itertools.product(GEOMETRIES, (0, 1), PERIODIC_CALLS):
            opts = dict(tune=0, nt=1, xcd=1, overlap=ov, deep_halo=dh, periodic_y=1, **plan)
            rc, text = dry(200, ny, bounds, transport, opts, calls, prec)
            runs += 1
            assert rc == 0, f"{opts} transport {transport} bounds {bounds} calls {calls}: rc {rc}\n{text[:3000]}"
    assert runs == len(STRIP_PLANS) * 6 * len(GEOMETRIES) * 2 * len(PERIODIC_CALLS)
    # with the samplers behind the force kernel (the frame reads two ghost rows per face, the probes two above)
    for bounds, ny in GEOMETRIES:
        opts = dict(tune=0, deep=1, periodic_y=1, stats=0, frames=1, probes=1, bodies=1)
        rc, text = dry(200, ny, bounds, 0, opts, [(13, 5), (1, 0), (20, 5)])
        assert rc == 0, text[:3000]


def test_a_lone_periodic_strip_wraps_through_device_copies(dry):  # noqa: F811
    rc, text = dry(200, 72, [(0, 72)], 0, dict(tune=0, deep=1, periodic_y=1), [(6, 0)], dump=1)
    assert rc == 0
    assert "copy buf 0: rows [66,72) of strip 0 -> rows [-6,0)" in text and "copy buf 0: rows [0,6) of strip 0 -> rows [72,78)" in text
    # without the option the same call is one launch and no transfer: the record of a walled domain is what it was
    rc, walled = dry(200, 72, [(0, 72)], 0, dict(tune=0, deep=1), [(6, 0)], dump=1)
    assert rc == 0 and "copy" not in walled and "rows [0,72)" in walled


def test_the_ring_waits_for_the_wrapped_neighbours_pull(dry):  # noqa: F811
    """Peer copies: strip 2 pulls strip 0's bottom rows, so strip 0 waits for strip 2's ev_comm before it overwrites them; without the
    waits (the test option of the walled groups) the checker names the race across the seam."""
    bounds = [(0, 100), (100, 100), (200, 100)]
    pairs = dict(tune=0, nt=1, xcd=1, overlap=0, deep_halo=1, fuse=3, pair_ty=12, periodic_y=1)
    rc, text = dry(200, 300, bounds, 0, pairs, [(40, 0)], dump=1)
    assert rc == 0, text[:2000]
    assert re.search(r"strip 0 main stream: wait ev_comm of strip 2", text) and re.search(r"strip 2 main stream: wait ev_comm of strip 0", text)
    assert re.search(r"strip 0 \w+ stream: copy buf \d: rows \[94,100\) of strip 2 -> rows \[-6,0\)", text)
    assert re.search(r"strip 2 \w+ stream: copy buf \d: rows \[0,6\) of strip 0 -> rows \[100,106\)", text)
    rc, text = dry(200, 300, bounds, 0, dict(pairs, debug_skip_pull_wait=1), [(40, 0)])
    assert rc > 0 and "RACE strip" in text and "copy buf" in text, text[:2000]
    rc, text = dry(200, 300, bounds, 0, dict(pairs, periodic_y=0), [(40, 0)], dump=1)          # walled: strip 0 never hears of strip 2
    assert rc == 0 and "wait ev_comm of strip 2" not in "\n".join(l for l in text.splitlines() if "strip 0 " in l.split(":")[0])


def test_two_strips_over_rccl_pair_up_in_posting_order(dry):  # noqa: F811
    """n == 2: both neighbours of a strip are the same peer, and RCCL pairs the k-th send to a peer with that peer's k-th receive from the
    sender. The record posts every northward message first, then every southward one, and states the pairing: strip 0's top rows
    arrive in strip 1's SOUTH ghost rows, its bottom rows in strip 1's NORTH ones."""
    rc, text = dry(200, 72, [(0, 36), (36, 36)], 1, dict(tune=0, deep=1, periodic_y=1), [(6, 0)], dump=1)
    assert rc == 0, text
    xfer = [l.split("stream: ", 1)[1] for l in text.splitlines() if "send buf" in l or "recv buf" in l]
    first = xfer[:8]
    assert first == ["send buf 0 rows [30,36) to strip 1", "recv buf 0 rows [-6,0) <- rows [30,36) of strip 1",
                     "send buf 0 rows [30,36) to strip 0", "recv buf 0 rows [-6,0) <- rows [30,36) of strip 0",
                     "send buf 0 rows [0,6) to strip 1", "recv buf 0 rows [36,42) <- rows [0,6) of strip 1",
                     "send buf 0 rows [0,6) to strip 0", "recv buf 0 rows [36,42) <- rows [0,6) of strip 0"], first
    owners = [int(re.match(r"#\d+ strip (\d+)", l).group(1)) for l in text.splitlines() if "send buf" in l or "recv buf" in l][:8]
    assert owners == [0, 0, 1, 1, 0, 0, 1, 1]
    # the k-th send of strip 0 to strip 1 meets strip 1's k-th receive from strip 0: top rows -> south ghost rows, bottom rows -> north ones
    sends01 = [l for l, o in zip(first, owners) if o == 0 and l.startswith("send") and l.endswith("to strip 1")]
    recvs10 = [l for l, o in zip(first, owners) if o == 1 and l.startswith("recv") and l.endswith("of strip 0")]
    assert [s.split(" to ")[0][5:] for s in sends01] == ["buf 0 rows [30,36)", "buf 0 rows [0,6)"]
    assert recvs10 == ["recv buf 0 rows [-6,0) <- rows [30,36) of strip 0", "recv buf 0 rows [36,42) <- rows [0,6) of strip 0"]
    # a walled group's record does not change: no pairing text, strip 0 sends north only
    rc, walled = dry(200, 72, [(0, 36), (36, 36)], 1, dict(tune=0, deep=1), [(6, 0)], dump=1)
    assert rc == 0 and " to strip" not in walled and "<-" not in walled


# ---- refusals that need no context ------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_context(lbm, dry):  # noqa: F811
    L = lbm.lib()
    assert L.lbm_set_periodic_y(None, 1) < 0 and b"lbm_set_periodic_y: null context" in L.lbm_last_error()
    assert L.lbm_get_periodic_y(None) == 0
    rc, text = dry(200, 72, [(0, 72)], 0, dict(tune=0, periodic_y=2), [(6, 0)])
    assert rc < 0 and "lbm_set_periodic_y: on = 2 (0 or 1 only)" in text
    # never a whole domain: the whole-domain-only shapes and the planar layout's transports
    rc, text = dry(200, 72, [(0, 72)], 0, dict(tune=0, deep=10, arith=1, periodic_y=1), [(6, 0)])
    assert rc < 0 and re.search(r"deep 10 .* exists for .* only", text), text
    rc, text = dry(200, 72, [(0, 72)], 0, dict(tune=0, deep=10, arith=1), [(6, 0)])
    assert rc == 0                                                            # (the walled whole domain runs it)
    for transport in (2, 3):
        rc, text = dry(200, 72, [(0, 72)], transport, dict(tune=0, deep=1, periodic_y=1), [(6, 0)])
        assert rc < 0 and "periodic_y=1 goes with transports 0 and 1" in text
    rc, text = dry(200, 22, [(0, 11), (11, 11)], 0, dict(tune=0, deep=1, periodic_y=1), [(6, 0)])
    assert rc < 0 and "at least 12 rows" in text
    # multi-process rings are not built: the pairing hook refuses them
    L.lbm_debug_p2p_matching.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                         C.c_char_p, C.c_int]
    b = (C.c_int * 4)(0, 36, 36, 36)
    cl = (C.c_int * 2)(6, 0)
    out = C.create_string_buffer(4096)
    assert L.lbm_debug_p2p_matching(200, 72, b, 2, 0, b"tune=0 deep=1 periodic_y=1", None, cl, 1, out, len(out)) < 0
    assert b"lbm_debug_p2p_matching: periodic_y=1" in L.lbm_last_error()
    assert L.lbm_debug_p2p_matching(200, 72, b, 2, 0, b"tune=0 deep=1", None, cl, 1, out, len(out)) == 0


def test_lbm_solver_refuses_bad_combinations_before_a_device_is_touched(solver, tmp_path):  # noqa: F811
    from tests.helpers import write_pgm

    def refused(args, what):
        pr = subprocess.run([solver, "--nx", "64", "--ny", "48", "--steps", "1", "--no-vtk", "--periodic-y"] + args, cwd=tmp_path,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert pr.returncode == 2, (args, pr.returncode, pr.stderr)
        assert len(pr.stderr.strip().splitlines()) == 1 and re.search(what, pr.stderr), (args, pr.stderr)
        assert pr.stdout == ""

    refused(["--walls", "free-slip"], "--periodic-y cannot be combined with a free-slip wall")
    refused(["--wall-north", "moving:0.02"], "--periodic-y cannot be combined with a moving:0.02 wall")
    refused(["--strips", "5"], "--periodic-y: 48 rows in 5 strip.s.: every strip needs at least 12 rows")
    labels = np.zeros((48, 64), np.uint8)
    labels[0:3, 10:14] = 1
    write_pgm(tmp_path / "bodies.pgm", labels)
    refused(["--obstacle-bodies", str(tmp_path / "bodies.pgm")], "--obstacle-bodies has a labelled cell on row 0")
