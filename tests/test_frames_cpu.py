"""Coarsened flow frames (lbm_frames_begin / k_frame), the part that needs no GPU: the exported symbols, the argument checks that
precede every device call, the place of the frame sample in the launch choreography, and the command line of lbm_solver.

The frame of iteration t reads P_t = buf[cur] at the iterations at which lbm_step evaluates the forces: the strip's rows and TWO ghost
rows per face — the ghost row next to a face for d ux / dy at the face, and the row beyond it, from which that ghost row's outlet cell
pulls. `lbm_debug_choreography` with the option `frames=1` records it as an operation of its own ("frame": reads rows
[-2, local_ny + 2) of buf[cur] on the main stream, writes a ring slot of its own) and checks it like every other access: no RACE with an
exchange that may still be writing the ghost rows, no STALE ghost row. Grids, strip bounds, plans and calls are those of
tests/test_choreography_cpu.py and tests/test_stats_cpu.py."""
import ctypes as C
import importlib
import itertools
import os
import re
import subprocess

import pytest

from tests import test_choreography_cpu as tc
from tests import test_choreography_split_cpu as ts
from tests.helpers import FRAME_PLANS, PKG, STAT_CALLS, geometries, ops_of, sample_points

LBM_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    lib = C.CDLL(pkg.lib_path())
    lib.lbm_frames_begin.argtypes = [C.c_void_p, C.c_int, C.c_int]      # (AttributeError on a library without frames)
    lib.lbm_frames_end.argtypes = [C.c_void_p]
    lib.lbm_frames_pending.argtypes = [C.c_void_p]
    lib.lbm_drain_frames.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
    lib.lbm_debug_choreography.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_int), C.c_int,
                                           C.c_int, C.c_char_p, C.c_int]
    lib.lbm_last_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def dry(L):
    out = C.create_string_buffer(1 << 22)

    def run(nx, ny, bounds, transport, options, calls, precision=0, dump=0):
        b = (C.c_int * (2 * len(bounds)))(*[v for p in bounds for v in p])
        cl = (C.c_int * (2 * len(calls)))(*[v for p in calls for v in p])
        rc = L.lbm_debug_choreography(nx, ny, b, len(bounds), precision, transport, " ".join(f"{k}={v}" for k, v in options.items()).encode(), cl,
                                      len(calls), dump, out, len(out))
        return rc, (out.value.decode() if rc >= 0 else L.lbm_last_error().decode())
    return run


def test_the_entry_points_are_exported_and_check_their_arguments(L):
    assert L.lbm_frames_begin(None, 4, 2) == LBM_ERR_ARG and b"initialised context" in L.lbm_last_error()
    assert L.lbm_frames_end(None) == LBM_ERR_ARG
    assert L.lbm_frames_pending(None) == LBM_ERR_ARG
    buf, ts_ = (C.c_float * 4)(), (C.c_int * 1)()
    assert L.lbm_drain_frames(None, ts_, buf, 1) == LBM_ERR_ARG


def test_the_binding_declares_the_entry_points():
    pkg = importlib.import_module(PKG)
    lib = pkg.lib()
    assert lib.lbm_frames_begin.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert lib.lbm_frames_end.argtypes == [C.c_void_p] and lib.lbm_frames_pending.argtypes == [C.c_void_p]
    assert lib.lbm_drain_frames.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
    for cls in (pkg.Context, pkg.Group):
        for name in ("frames_begin", "frames_end", "frames_pending", "drain_frames"):
            assert callable(getattr(cls, name)), (cls, name)


def test_the_frame_sample_is_ordered_and_fresh_in_every_schedule(dry):
    """frames=1: 0 violations on the strip layouts and call sequences the statistics sample is checked on, transports 0 and 3, every
    overlap x deep_halo schedule; the record shows one "frame" operation per strip at exactly the force points, each behind the
    force kernel of its strip and iteration; without the option the record is that of a run without frames."""
    runs = 0
    for (plan, prec), dh, ov in itertools.product(FRAME_PLANS, (0, 1, 2), (0, 1, 2)):
        opts = dict(tune=0, nt=1, xcd=1, overlap=ov, deep_halo=dh, trailing_pair=0, **plan)
        for transport, bounds, ny in geometries():
            if transport not in (0, 3):
                continue
            for calls in STAT_CALLS:
                rc, text = dry(256, ny, bounds, transport, dict(opts, frames=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} transport {transport} bounds {bounds} calls {calls}: rc {rc}\n{text[:3000]}"
                forces, frames = ops_of(text, "forces"), ops_of(text, "frame")
                for k in range(len(bounds)):
                    assert [t for s, t in frames if s == k] == [t for s, t in forces if s == k] == sample_points(calls, 0)
                lines = text.splitlines()
                for i, ln in enumerate(lines):
                    if ": frame t=" in ln:      # directly behind the force kernel of the same strip and iteration
                        prev = lines[i - 1]
                        assert ": forces t=" in prev and ln.split(" main")[0].split(" ", 1)[1] == prev.split(" main")[0].split(" ", 1)[1], lines[i - 1:i + 1]
                        assert re.search(r"t=(\d+) ", ln).group(1) == re.search(r"t=(\d+) ", prev).group(1)
                rc0, plain = dry(256, ny, bounds, transport, opts, calls, prec, dump=1)
                assert rc0 == 0 and ": frame" not in plain
                strip_no = lambda s: [re.sub(r"^#\d+ ", "", ln) for ln in s.splitlines() if ": frame t=" not in ln]
                assert strip_no(text) == strip_no(plain)
    assert runs > 300


def test_the_frame_sample_beside_statistics_and_bodies_on_every_transport(dry):
    """All three samples behind one force kernel, transports 0-3, both plans."""
    for (plan, prec), (transport, bounds, ny) in itertools.product(FRAME_PLANS, geometries()):
        opts = dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, trailing_pair=0, stats=0, bodies=1, frames=1, **plan)
        rc, text = dry(256, ny, bounds, transport, opts, [(50, 13)], prec, dump=1)
        assert rc == 0, f"{opts} transport {transport} bounds {bounds}: rc {rc}\n{text[:3000]}"
        assert len(ops_of(text, "frame")) == len(ops_of(text, "stats")) == len(ops_of(text, "forces")) == 4 * len(bounds)


def test_the_frame_sample_reads_two_ghost_rows_per_face(dry):
    b, ny = tc.strips_of((13, 24, 17))
    rc, text = dry(256, ny, b, 0, dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, deep=7, arith=1, frames=1), [(31, 7)], dump=1)
    assert rc == 0, text
    assert "strip 1 main stream: frame t=7 reads buf" in text and "rows [-2,26), writes its ring slot" in text, text


def test_a_ghost_row_that_is_not_refreshed_makes_the_frame_stale(dry):
    """Negative control: with the exchange cut ("skip_exchange") the frame of a middle rank finds old ghost rows, and the checker names it."""
    rc, text = dry(256, 384, [(128, 128)], 2, dict(tune=0, nt=1, xcd=1, overlap=0, deep_halo=0, fuse=1, skip_exchange=1, frames=1), [(3, 2)])
    assert rc > 0 and "STALE strip 0 buffer" in text and "frame t=2" in text, text


def test_split_plans_sample_on_the_joined_main_stream(dry):
    runs = 0
    for (plan, prec), sp in itertools.product(ts.PLANS, (3, 4)):
        opts = dict(tune=0, nt=0, xcd=1, alternate=1, trailing_pair=0, split=sp, split_min=1, **plan)
        for ny in (24, 133, 1024):
            for calls in ([(31, 7)], [(5, 0), (20, 0), (97, 10)]):
                rc, text = dry(256, ny, [(0, ny)], 0, dict(opts, frames=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
                assert [t for _, t in ops_of(text, "frame")] == sample_points(calls, 0)
    assert runs > 20


@pytest.mark.parametrize("value", [0, -1, 65])
def test_a_stride_out_of_range_is_refused_by_the_option(dry, value):
    rc, text = dry(256, 64, [(0, 64)], 0, dict(tune=0, fuse=1, frames=value), [(3, 1)])
    assert rc == LBM_ERR_ARG and "frames (the stride k) must be in 1..64" in text, text


# ---- lbm_solver --frame-stride ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "lbm_solver")
    assert os.path.exists(exe), "host/lbm_solver was not built"
    return exe


def test_help_documents_the_flag(solver):
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--frame-stride K" in r.stdout and "vorticity" in r.stdout


@pytest.mark.parametrize("args, message", [
    (["--frame-stride", "x"], "--frame-stride: 'x' is not a whole number in 1..64"),
    (["--frame-stride", "2.5"], "--frame-stride: '2.5' is not a whole number in 1..64"),
    (["--frame-stride", "0"], "--frame-stride: '0' is not a whole number in 1..64"),
    (["--frame-stride", "65"], "--frame-stride: '65' is not a whole number in 1..64"),
    (["--frame-stride"], "missing value for --frame-stride"),
    (["--frame-stride", "5"], "--frame-stride: 5 does not divide the lattice 128x48"),
    (["--frame-stride", "32"], "--frame-stride: 32 does not divide the lattice 128x48"),
    (["--frame-stride", "4", "--strips", "5"], "--frame-stride: 4 does not divide the rows of strip 0 of 5"),
    (["--frame-stride", "16", "--gpus", "2"], "--frame-stride: 16 does not divide the rows of strip 0 of 2"),
    (["--frame-stride", "4", "--output-frequency", "0"], "--frame-stride needs --output-frequency > 0")])
def test_lbm_solver_refuses_a_bad_frame_stride_before_opening_a_device(solver, tmp_path, args, message):
    """Exit code 2, the reason named, no device banner and no file written — with no device visible at all."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([solver, "--nx", "128", "--ny", "48", "--steps", "10", "--output-frequency", "5"] + args, cwd=tmp_path, capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert message in r.stderr and "unknown option" not in r.stderr, r.stderr
    assert "MI355X HIP Grid" not in r.stdout
    assert os.listdir(tmp_path) == []


def test_lbm_solver_accepts_a_valid_frame_stride(solver, tmp_path):
    """Positive control: a divisor with a cadence passes the command line. Without a device the run then ends at the first device
    call (exit code 1); with one it completes. Either way it is not the exit code 2 of a refused option."""
    r = subprocess.run([solver, "--nx", "128", "--ny", "48", "--steps", "10", "--output-frequency", "5", "--frame-stride", "4", "--strips", "3",
                        "--no-vtk", "--no-tune", "--quiet"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)
    assert "frame-stride" not in r.stderr and "unknown option" not in r.stderr, r.stderr
    if r.returncode == 0:
        assert sorted(os.listdir(tmp_path / "vtk_output")) == ["frame_000000.vtk", "frame_000005.vtk"]
