"""Time-averaged statistics (lbm_stats_begin / k_stats), the part that needs no GPU: the exported symbols, the argument checks, the
place of the sample in the launch choreography, and the command line of lbm_solver.

The sample of iteration t reads P_t = buf[cur] at the iterations at which lbm_step evaluates the forces; on the inlet and outlet
columns of a strip's first and last row it pulls from ONE ghost row per face. `lbm_debug_choreography` with the option `stats=N` records
it as an operation of its own ("stats": reads rows [-1, local_ny + 1) of buf[cur] on the main stream, writes the strip's accumulators)
and checks it like every other access: no RACE with an exchange that may still be writing the ghost rows, no STALE ghost row, and every
sample ordered behind the one before it on the accumulators. Grids, strip bounds, plans and calls are those of
tests/test_choreography_cpu.py and tests/test_choreography_split_cpu.py."""
import ctypes as C
import importlib
import itertools
import os
import re
import subprocess

import pytest

from tests import test_choreography_cpu as tc
from tests import test_choreography_split_cpu as ts
from tests.helpers import PKG, STAT_CALLS, geometries, ops_of, sample_points
SYMBOLS = ("lbm_stats_begin", "lbm_stats_end", "lbm_stats_samples", "lbm_get_stat_sums", "lbm_stats_restore")
LBM_ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    lib = C.CDLL(pkg.lib_path())
    for s in SYMBOLS:          # (AttributeError on a library without statistics)
        getattr(lib, s)
    lib.lbm_stats_begin.argtypes = [C.c_void_p, C.c_int]
    lib.lbm_get_stat_sums.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.lbm_stats_restore.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    lib.lbm_stats_end.argtypes = [C.c_void_p]
    lib.lbm_stats_samples.argtypes = [C.c_void_p]
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
    assert L.lbm_stats_begin(None, 0) == LBM_ERR_ARG
    buf = (C.c_double * 6)()
    assert L.lbm_get_stat_sums(None, buf) == LBM_ERR_ARG
    assert L.lbm_stats_restore(None, buf, 0) == LBM_ERR_ARG
    assert L.lbm_stats_end(None) == LBM_ERR_ARG
    assert L.lbm_stats_samples(None) == LBM_ERR_ARG


def test_the_sample_is_ordered_and_fresh_in_every_schedule(dry):
    """stats=0 / stats=N: 0 violations for transports 0-3, every overlap x deep_halo schedule and every plan family; the record shows
    one "stats" operation per strip at exactly the force points at or after N; and without the option the record is the one of a run
    that never heard of statistics (compared in this test, run against run)."""
    runs = 0
    for (plan, prec), dh, ov in itertools.product(tc.PLANS, (0, 1, 2), (0, 1, 2)):
        opts = dict(tune=0, nt=1, xcd=1, overlap=ov, deep_halo=dh, trailing_pair=0, **plan)
        for transport, bounds, ny in geometries():
            for calls in STAT_CALLS:
                for from_step in (0, 9):
                    rc, text = dry(256, ny, bounds, transport, dict(opts, stats=from_step), calls, prec, dump=1)
                    runs += 1
                    assert rc == 0, f"{opts} stats={from_step} transport {transport} bounds {bounds} calls {calls}: rc {rc}\n{text[:3000]}"
                    forces, stats = ops_of(text, "forces"), ops_of(text, "stats")
                    for k in range(len(bounds)):
                        assert [t for s, t in forces if s == k] == sample_points(calls, 0)
                        assert [t for s, t in stats if s == k] == sample_points(calls, from_step), (opts, transport, bounds, calls, from_step)
                    # every sample directly follows the force kernel of its strip and iteration
                    lines = text.splitlines()
                    for i, ln in enumerate(lines):
                        if ": stats t=" in ln:
                            assert ": forces t=" in lines[i - 1] and ln.split(" main")[0].split(" ", 1)[1] == lines[i - 1].split(" main")[0].split(" ", 1)[1], lines[i - 1:i + 1]
                rc0, plain = dry(256, ny, bounds, transport, opts, calls, prec, dump=1)
                assert rc0 == 0 and ": stats" not in plain
                # the record with statistics, minus the sample operations, is the record without (operation numbers aside)
                strip_no = lambda s: [re.sub(r"^#\d+ ", "", ln) for ln in s.splitlines() if ": stats t=" not in ln]
                assert strip_no(text) == strip_no(plain)
    assert runs > 5000


def test_the_sample_reads_one_ghost_row_per_face(dry):
    b, ny = tc.strips_of((13, 24, 17))
    rc, text = dry(256, ny, b, 0, dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, deep=7, arith=1, stats=0), [(31, 7)], dump=1)
    assert rc == 0, text
    assert "strip 1 main stream: stats t=7 reads buf" in text and "rows [-1,25), writes the accumulators" in text, text


def test_a_ghost_row_that_is_not_refreshed_makes_the_sample_stale(dry):
    """Negative control: with the exchange cut ("skip_exchange") the sample of a middle rank finds an old ghost row, and the checker names it."""
    rc, text = dry(256, 384, [(128, 128)], 2, dict(tune=0, nt=1, xcd=1, overlap=0, deep_halo=0, fuse=1, skip_exchange=1, stats=0), [(3, 2)])
    assert rc > 0 and "STALE strip 0 buffer" in text and "stats t=2" in text, text


def test_split_plans_sample_on_the_joined_main_stream(dry):
    """The whole-domain "split" 3 / 4 plans: the sample follows the join of the two streams, like the force kernel."""
    runs = 0
    for (plan, prec), sp, smin in itertools.product(ts.PLANS, (3, 4), (1, 8)):
        opts = dict(tune=0, nt=0, xcd=1, alternate=1, trailing_pair=0, split=sp, split_min=smin, **plan)
        for ny in (24, 64, 133, 256, 1024):
            for calls in ([(31, 7)], [(97, 31), (5, 0)], [(5, 0), (20, 0), (97, 10)], [(120, 30)]):
                rc, text = dry(256, ny, [(0, ny)], 0, dict(opts, stats=0), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
                assert [t for _, t in ops_of(text, "stats")] == sample_points(calls, 0)
                rc0, plain = dry(256, ny, [(0, ny)], 0, opts, calls, prec, dump=1)
                assert rc0 == 0 and ": stats" not in plain and len(plain.splitlines()) == len(text.splitlines()) - len(sample_points(calls, 0))
    assert runs > 300


def test_a_negative_start_is_refused_by_the_option(dry):
    rc, text = dry(256, 64, [(0, 64)], 0, dict(tune=0, fuse=1, stats=-1), [(3, 1)])
    assert rc == LBM_ERR_ARG and "stats (the first step sampled) must be >= 0" in text, text


# ---- lbm_solver --stats-start ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    exe = os.path.join(os.path.dirname(pkg.__file__), "host", "lbm_solver")
    assert os.path.exists(exe), "host/lbm_solver was not built"
    return exe


@pytest.mark.parametrize("args, message", [
    (["--stats-start", "-3"], "--stats-start: '-3' is not a step number >= 0"),
    (["--stats-start", "x"], "--stats-start: 'x' is not a step number >= 0"),
    (["--stats-start"], "missing value for --stats-start"),
    (["--stats-start", "0", "--output-frequency", "0"], "--stats-start needs --output-frequency > 0")])
def test_lbm_solver_refuses_a_bad_stats_start_before_opening_a_device(solver, tmp_path, args, message):
    """Each refusal names its own reason: an executable that does not know the flag at all says "unknown option" and is told apart."""
    r = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10"] + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert message in r.stderr and "unknown option" not in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


def test_lbm_solver_accepts_a_valid_stats_start(solver, tmp_path):
    """Positive control: a step number with a cadence passes the command line. Without a device the run then ends at the first
    device call (exit code 1); with one it completes. Either way it is not the exit code 2 of a refused option."""
    r = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10", "--output-frequency", "5", "--stats-start", "5", "--no-vtk", "--no-tune",
                        "--quiet"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)
    assert "stats-start" not in r.stderr and "unknown option" not in r.stderr, r.stderr
    if r.returncode == 0:
        assert os.path.exists(tmp_path / "mean_fields.csv")
