"""Point probes (lbm_probes_begin / k_probes), the part that needs no GPU: the exported symbols and their argument checks, the probe
table (ownership by strip, clamping at the domain's edge, exact weights) against a numpy restatement, the place of the probe sample in
the launch choreography, and the probe points of lbm_solver's command line (host/lbm/probes.hpp) through a stand-alone client, built
once as the Makefile builds it and once with -fsanitize=address,undefined.

The probe sample of iteration t reads P_t = buf[cur] at the iterations at which lbm_step evaluates the forces: the strip's rows, the
ghost row below (the pull of an inlet / outlet cell of row 0) and TWO ghost rows above (y1 of a probe on the strip's last row, and the
row that ghost row's inlet / outlet cell pulls from). `lbm_debug_choreography` with the option `probes=1` records it as an operation
of its own ("probes": reads rows [-1, local_ny + 2) of buf[cur] on the main stream, writes a ring slot of its own). Grids, strip bounds,
plans and calls are those tests/test_frames_cpu.py enumerates for the frame sample."""
import ctypes as C
import importlib
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import test_choreography_cpu as tc
from tests import test_choreography_split_cpu as ts
from tests.helpers import FRAME_PLANS, PKG, ROOT, STAT_CALLS, geometries, ops_of, sample_points

LBM_ERR_ARG = -1
PROBES_MAX = 65536
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def L():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    lib = C.CDLL(pkg.lib_path())
    lib.lbm_probes_begin.argtypes = [C.c_void_p, dp, C.c_int, C.c_int]      # (AttributeError on a library without probes)
    lib.lbm_probes_end.argtypes = [C.c_void_p]
    lib.lbm_probes_count.argtypes = [C.c_void_p]
    lib.lbm_probes_pending.argtypes = [C.c_void_p]
    lib.lbm_drain_probes.argtypes = [C.c_void_p, ip, dp, C.c_int]
    lib.lbm_debug_probe_table.argtypes = [dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, dp, ip]
    lib.lbm_debug_choreography.argtypes = [C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_char_p, ip, C.c_int, C.c_int, C.c_char_p, C.c_int]
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
    xy = (C.c_double * 2)(1.0, 1.0)
    assert L.lbm_probes_begin(None, xy, 1, 2) == LBM_ERR_ARG and b"initialised context" in L.lbm_last_error()
    assert L.lbm_probes_end(None) == LBM_ERR_ARG
    assert L.lbm_probes_count(None) == LBM_ERR_ARG
    assert L.lbm_probes_pending(None) == LBM_ERR_ARG
    buf, ts_ = (C.c_double * 3)(), (C.c_int * 1)()
    assert L.lbm_drain_probes(None, ts_, buf, 1) == LBM_ERR_ARG


def test_the_binding_declares_the_entry_points():
    pkg = importlib.import_module(PKG)
    lib = pkg.lib()
    assert lib.lbm_probes_begin.argtypes == [C.c_void_p, dp, C.c_int, C.c_int]
    assert lib.lbm_probes_end.argtypes == [C.c_void_p] and lib.lbm_probes_pending.argtypes == [C.c_void_p] and lib.lbm_probes_count.argtypes == [C.c_void_p]
    assert lib.lbm_drain_probes.argtypes == [C.c_void_p, ip, dp, C.c_int]
    for cls in (pkg.Context, pkg.Group):
        for name in ("probes_begin", "probes_end", "probes_pending", "probes_count", "drain_probes"):
            assert callable(getattr(cls, name)), (cls, name)
    assert pkg.Context.PROBES_MAX == PROBES_MAX
    header = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    assert re.search(r"#define LBM_PROBES_MAX\s+65536\b", header)


# ---- 1. the probe table ------------------------------------------------------------------------------------------------------------
NX, NY = 128, 32
POINTS = [(0.0, 0.0), (NX - 1.0, 0.0), (0.0, NY - 1.0), (NX - 1.0, NY - 1.0),      # the four corners of the domain
          (63.5, 15.5), (NX - 1.0, 7.25), (5.0, 15.5),                           # (5, 15.5) straddles the 16 + 16 face
          (40.0, 15.0), (40.0, 9.0),                                             # nodes on the last row of the lower strip (16 + 16, 10 + 22)
          (0.25, 9.75), (126.5, 30.125), (17.0, 3.0)]
LAYOUTS = [[(0, 32)], [(0, 16), (16, 16)], [(0, 10), (10, 22)]]


def table(L, pts, nx, ny, y_start, rows):
    n = len(pts)
    xy = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    cells, w, own = np.full((n, 4), -7, dtype=np.int32), np.full((n, 2), -7.0), np.full(n, -7, dtype=np.int32)
    rc = L.lbm_debug_probe_table(xy.ctypes.data_as(dp), n, nx, ny, y_start, rows, cells.ctypes.data_as(ip), w.ctypes.data_as(dp), own.ctypes.data_as(ip))
    return rc, cells, w, own


def numpy_table(pts, nx, ny, y_start, rows):
    """The definition, restated: x0 = floor(px), fx = px - x0, x1 = min(x0 + 1, nx - 1); y likewise with ny - 1; the owner is the strip
    whose rows hold floor(py); y in local rows; a probe that is not owned has cell (0, 0), weights 0 and clamps from there."""
    xy = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    x0, y0 = np.floor(xy[:, 0]).astype(np.int64), np.floor(xy[:, 1]).astype(np.int64)
    own = (y0 >= y_start) & (y0 < y_start + rows)
    fx, fy = np.where(own, xy[:, 0] - x0, 0.0), np.where(own, xy[:, 1] - y0, 0.0)
    x0 = np.where(own, x0, 0)
    y0g = np.where(own, y0, y_start)
    cells = np.stack([x0, y0g - y_start, np.minimum(x0 + 1, nx - 1), np.minimum(y0g + 1, ny - 1) - y_start], axis=1)
    return cells.astype(np.int32), np.stack([fx, fy], axis=1), own.astype(np.int32)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["whole", "16+16", "10+22"])
def test_the_probe_table_equals_the_numpy_restatement(L, layout):
    owners = np.zeros(len(POINTS), dtype=int)
    for y_start, rows in layout:
        rc, cells, w, own = table(L, POINTS, NX, NY, y_start, rows)
        assert rc == len(POINTS), L.lbm_last_error()
        rcells, rw, rown = numpy_table(POINTS, NX, NY, y_start, rows)
        assert np.array_equal(own, rown), (y_start, rows, own, rown)
        assert np.array_equal(cells, rcells), (y_start, rows, cells, rcells)
        assert np.array_equal(w, rw), (y_start, rows, w, rw)                     # exact: px - floor(px) is representable
        owners += own
        for j, (px, py) in enumerate(POINTS):
            if not own[j]:
                assert list(cells[j, :2]) == [0, 0] and list(w[j]) == [0.0, 0.0]
                continue
            x0, y0, x1, y1 = (int(v) for v in cells[j])
            assert 0 <= x0 <= x1 <= NX - 1 and x1 - x0 <= 1 and 0 <= y0 < rows and 0 <= y1 - y0 <= 1
            assert y_start + y1 <= NY - 1                                        # clamped at the DOMAIN's edge, not at the strip's
            assert x0 + w[j, 0] == px and y_start + y0 + w[j, 1] == py
            if px == int(px) and py == int(py):                                  # a node: no neighbour has a weight
                assert w[j, 0] == 0.0 and w[j, 1] == 0.0
            if w[j, 0] != 0.0:
                assert x1 == x0 + 1
            if w[j, 1] != 0.0:
                assert y1 == y0 + 1                                              # (may be `rows`: the ghost row next to the north face)
    assert np.array_equal(owners, np.ones(len(POINTS), dtype=int)), owners       # each probe is owned by exactly one strip


def test_the_face_straddling_probe_reads_the_owners_north_ghost_row(L):
    """(5, 15.5) on 16 + 16: the lower strip owns it, y0 is its last row and y1 the ghost row beyond; the node (40, 15) on that same row
    has no weight on a neighbour, so it reads no ghost row; the corners clamp at the domain's edge."""
    rc, cells, w, own = table(L, POINTS, NX, NY, 0, 16)
    j = POINTS.index((5.0, 15.5))
    assert own[j] == 1 and list(cells[j]) == [5, 15, 6, 16] and list(w[j]) == [0.0, 0.5]
    j = POINTS.index((40.0, 15.0))
    assert own[j] == 1 and list(cells[j][:2]) == [40, 15] and list(w[j]) == [0.0, 0.0]
    rc, cells, w, own = table(L, POINTS, NX, NY, 16, 16)
    assert own[POINTS.index((5.0, 15.5))] == 0 and own[POINTS.index((40.0, 15.0))] == 0
    j = POINTS.index((NX - 1.0, NY - 1.0))
    assert own[j] == 1 and list(cells[j]) == [NX - 1, 15, NX - 1, 15] and list(w[j]) == [0.0, 0.0]
    j = POINTS.index((126.5, 30.125))
    assert own[j] == 1 and list(cells[j]) == [126, 14, 127, 15] and list(w[j]) == [0.5, 0.125]


# ---- 2. argument errors of the table hook ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pts, text", [
    ([(-0.5, 3.0)], "probe 0: x = -0.5 outside the domain 0..127"),
    ([(1.0, 1.0), (127.5, 3.0)], "probe 1: x = 127.5 outside the domain 0..127"),
    ([(3.0, 31.0000001)], "probe 0: y = 31.0000001"),
    ([(3.0, -1e-9)], "probe 0: y = -1"),
    ([(float("nan"), 3.0)], "probe 0: (nan, 3) is not finite"),
    ([(1.0, 1.0), (2.0, 2.0), (3.0, float("inf"))], "probe 2: (3, inf) is not finite")])
def test_the_table_hook_names_a_bad_coordinate(L, pts, text):
    rc, *_ = table(L, pts, NX, NY, 0, NY)
    assert rc == LBM_ERR_ARG and text in L.lbm_last_error().decode(), L.lbm_last_error()


def test_the_table_hook_refuses_a_bad_count_or_strip(L):
    xy = np.zeros((PROBES_MAX + 1, 2))
    q = xy.ctypes.data_as(dp)
    assert L.lbm_debug_probe_table(q, 0, NX, NY, 0, NY, None, None, None) == LBM_ERR_ARG and b"n = 0 < 1" in L.lbm_last_error()
    assert L.lbm_debug_probe_table(q, -3, NX, NY, 0, NY, None, None, None) == LBM_ERR_ARG and b"n = -3 < 1" in L.lbm_last_error()
    assert L.lbm_debug_probe_table(q, PROBES_MAX + 1, NX, NY, 0, NY, None, None, None) == LBM_ERR_ARG
    assert b"n = 65537 > LBM_PROBES_MAX = 65536" in L.lbm_last_error()
    assert L.lbm_debug_probe_table(q, PROBES_MAX, NX, NY, 0, NY, None, None, None) == PROBES_MAX      # the largest n, outputs optional
    assert L.lbm_debug_probe_table(None, 1, NX, NY, 0, NY, None, None, None) == LBM_ERR_ARG and b"null" in L.lbm_last_error()
    assert L.lbm_debug_probe_table(q, 1, NX, NY, 20, 16, None, None, None) == LBM_ERR_ARG and b"outside the lattice" in L.lbm_last_error()


# ---- 3. the probe sample in the launch choreography --------------------------------------------------------------------------------
def test_the_probe_sample_is_ordered_and_fresh_in_every_schedule(dry):
    """probes=1: 0 violations on the strip layouts and call sequences the frame sample is checked on, transports 0 and 3, every
    overlap x deep_halo schedule; one "probes" operation per strip at exactly the force points, each directly behind the force kernel of
    its strip and iteration; without the option the record is that of a run without probes."""
    runs = 0
    for (plan, prec), dh, ov in itertools.product(FRAME_PLANS, (0, 1, 2), (0, 1, 2)):
        opts = dict(tune=0, nt=1, xcd=1, overlap=ov, deep_halo=dh, trailing_pair=0, **plan)
        for transport, bounds, ny in geometries():
            if transport not in (0, 3):
                continue
            for calls in STAT_CALLS:
                rc, text = dry(256, ny, bounds, transport, dict(opts, probes=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} transport {transport} bounds {bounds} calls {calls}: rc {rc}\n{text[:3000]}"
                forces, probes = ops_of(text, "forces"), ops_of(text, "probes")
                for k in range(len(bounds)):
                    assert [t for s, t in probes if s == k] == [t for s, t in forces if s == k] == sample_points(calls, 0)
                lines = text.splitlines()
                for i, ln in enumerate(lines):
                    if ": probes t=" in ln:      # directly behind the force kernel of the same strip and iteration
                        prev = lines[i - 1]
                        assert ": forces t=" in prev and ln.split(" main")[0].split(" ", 1)[1] == prev.split(" main")[0].split(" ", 1)[1], lines[i - 1:i + 1]
                        assert re.search(r"t=(\d+) ", ln).group(1) == re.search(r"t=(\d+) ", prev).group(1)
                rc0, plain = dry(256, ny, bounds, transport, opts, calls, prec, dump=1)
                assert rc0 == 0 and ": probes" not in plain
                strip_no = lambda s: [re.sub(r"^#\d+ ", "", ln) for ln in s.splitlines() if ": probes t=" not in ln]
                assert strip_no(text) == strip_no(plain)
    assert runs > 300


def test_the_probe_sample_beside_every_other_sample_on_every_transport(dry):
    """All four samples behind one force kernel, transports 0-3, both plans; the probes come last."""
    for (plan, prec), (transport, bounds, ny) in itertools.product(FRAME_PLANS, geometries()):
        opts = dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, trailing_pair=0, stats=0, bodies=1, frames=1, probes=1, **plan)
        rc, text = dry(256, ny, bounds, transport, opts, [(50, 13)], prec, dump=1)
        assert rc == 0, f"{opts} transport {transport} bounds {bounds}: rc {rc}\n{text[:3000]}"
        assert len(ops_of(text, "probes")) == len(ops_of(text, "frame")) == len(ops_of(text, "stats")) == len(ops_of(text, "forces")) == 4 * len(bounds)
        lines = text.splitlines()
        for i, ln in enumerate(lines):
            if ": probes t=" in ln:
                assert ": frame t=" in lines[i - 1] and ": stats t=" in lines[i - 2] and ": body forces t=" in lines[i - 3] and ": forces t=" in lines[i - 4]


def test_the_probe_sample_reads_one_ghost_row_below_and_two_above(dry):
    b, ny = tc.strips_of((13, 24, 17))
    rc, text = dry(256, ny, b, 0, dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, deep=7, arith=1, probes=1), [(31, 7)], dump=1)
    assert rc == 0, text
    assert "strip 1 main stream: probes t=7 reads buf" in text and "rows [-1,26), writes its ring slot" in text, text


def test_a_ghost_row_that_is_not_refreshed_makes_the_probe_sample_stale(dry):
    """Negative control, the one of tests/test_frames_cpu.py: with the exchange cut ("skip_exchange") the probe sample of a middle rank
    finds old ghost rows, and the checker names the probe read."""
    opts = dict(tune=0, nt=1, xcd=1, overlap=0, deep_halo=0, fuse=1, skip_exchange=1)
    rc, text = dry(256, 384, [(128, 128)], 2, dict(opts, probes=1), [(3, 2)])
    assert rc > 0 and "STALE strip 0 buffer" in text and "probes t=2" in text, text
    stale = re.findall(r"STALE strip 0 buffer \d row (-?\d+) holds.*\n\s+#\d+ strip 0 main stream: probes t=2", text)
    assert sorted(int(r) for r in stale) == [-1, 128, 129], text      # the rows the sample reads beyond the strip's own
    rc, text = dry(256, 384, [(128, 128)], 2, dict(opts, skip_exchange=0, probes=1), [(3, 2)])
    assert rc == 0, text


def test_split_plans_sample_on_the_joined_main_stream(dry):
    runs = 0
    for (plan, prec), sp in itertools.product(ts.PLANS, (3, 4)):
        opts = dict(tune=0, nt=0, xcd=1, alternate=1, trailing_pair=0, split=sp, split_min=1, **plan)
        for ny in (24, 133, 1024):
            for calls in ([(31, 7)], [(5, 0), (20, 0), (97, 10)]):
                rc, text = dry(256, ny, [(0, ny)], 0, dict(opts, probes=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
                assert [t for _, t in ops_of(text, "probes")] == sample_points(calls, 0)
    assert runs > 20


# ---- 4. the probe points of the command line (host/lbm/probes.hpp) ------------------------------------------------------------------
HOST = os.path.join(ROOT, PKG, "host")
PROBE_FILE = "# a rake behind the cylinder\n40 2\n40.5\t11.25   # tab-separated, with a comment\n\n   \n1e1 2.5e0\n127 31"      # (no final newline)
FILE_POINTS = [(40.0, 2.0), (40.5, 11.25), (10.0, 2.5), (127.0, 31.0)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probes_check(request, tmp_path_factory):
    """host/probes_check, a stand-alone program with its own main: as the Makefile builds it, and built with
    -fsanitize=address,undefined (run stand-alone; nothing loaded into Python is run under a sanitizer)."""
    if request.param == "plain":
        subprocess.check_call(["make", "-s", "-C", HOST])
        exe = os.path.join(HOST, "probes_check")
    else:
        exe = str(tmp_path_factory.mktemp("probes_check") / "probes_check_san")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                               "-static-libasan", "-static-libubsan",      # (the runtime inside the program: nothing to preload, no link order)
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe, os.path.join(HOST, "probes_check.cpp")])
    assert os.path.exists(exe)

    def run(*args, cwd=None):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60, cwd=cwd, env=env)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        return r
    return run


def points_of(r):
    assert r.returncode == 0, (r.returncode, r.stderr)
    return [tuple(float(v) for v in ln.split()) for ln in r.stdout.splitlines()]


def line_points(x0, y0, x1, y1, n):
    """--probe-line as documented: point j = p0 + (p1 - p0) * j / (n - 1), the product first; the end points themselves."""
    def at(a, b, j):
        if j == 0:
            return a
        if j == n - 1:
            return b
        return min(max(a + (b - a) * float(j) / float(n - 1), min(a, b)), max(a, b))
    return [(at(x0, x1, j), at(y0, y1, j)) for j in range(n)]


def test_probe_line_expansion(probes_check):
    assert points_of(probes_check(128, 32, "--probe-line", 40, 2, 40, 29, 10)) == [(40.0, 2.0 + 3.0 * j) for j in range(10)]
    assert points_of(probes_check(128, 32, "--probe-line", 0, 0, 127, 31, 3)) == [(0.0, 0.0), (63.5, 15.5), (127.0, 31.0)]
    assert points_of(probes_check(128, 32, "--probe-line", 5, 6, 100, 7, 1)) == [(5.0, 6.0)]
    assert points_of(probes_check(128, 32, "--probe-line", 100.25, 31, 100.25, 0, 64)) == line_points(100.25, 31.0, 100.25, 0.0, 64)
    got = points_of(probes_check(128, 32, "--probe-line", 0.1, 0.3, 126.9, 30.7, 7))
    assert got == line_points(0.1, 0.3, 126.9, 30.7, 7) and got[0] == (0.1, 0.3) and got[-1] == (126.9, 30.7)
    big = points_of(probes_check(4096, 1024, "--probe-line", 0, 0, 4095, 1023, PROBES_MAX))
    assert len(big) == PROBES_MAX and big == line_points(0.0, 0.0, 4095.0, 1023.0, PROBES_MAX)


def test_probe_file_parsing_and_combination(probes_check, tmp_path):
    f = tmp_path / "probes.txt"
    f.write_text(PROBE_FILE)
    assert points_of(probes_check(128, 32, "--probes", f)) == FILE_POINTS
    both = points_of(probes_check(128, 32, "--probe-line", 1, 1, 3, 1, 3, "--probes", f, "--probe-line", 9, 9, 9, 9, 2))
    assert both == [(1.0, 1.0), (2.0, 1.0), (3.0, 1.0)] + FILE_POINTS + [(9.0, 9.0), (9.0, 9.0)]      # the order of the options


@pytest.mark.parametrize("content, message", [
    ("1 2\n3\n", "line 2: 1 numbers, a probe is `x y`"),
    ("1 2 3\n", "line 1: 3 numbers, a probe is `x y`"),
    ("1 2\n4 x7\n", "line 2: 'x7' is not a number"),
    ("1 nan\n", "line 1: 'nan' is not finite"),
    ("# nothing\n\n", "no probe point"),
    ("1 2\n128 3\n", "probe 1: (128, 3) outside the domain 0..127 x 0..31"),
    ("1 -0.5\n", "probe 0: (1, -0.5) outside the domain")])
def test_a_bad_probe_file_is_refused_with_the_reason(probes_check, tmp_path, content, message):
    f = tmp_path / "bad.txt"
    f.write_text(content)
    r = probes_check(128, 32, "--probes", f)
    assert r.returncode == 2 and message in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("args, message", [
    (["--probe-line", "1", "2", "3", "4"], "--probe-line takes five values"),
    (["--probe-line", "1", "2", "3", "4", "0"], "'0' is not a number of points in 1..65536"),
    (["--probe-line", "1", "2", "3", "4", "65537"], "'65537' is not a number of points in 1..65536"),
    (["--probe-line", "1", "2", "3", "4", "2.5"], "'2.5' is not a number of points"),
    (["--probe-line", "1", "a", "3", "4", "2"], "--probe-line: 'a' is not a number"),
    (["--probe-line", "1", "2", "3", "32", "2"], "probe 1: (3, 32) outside the domain"),
    (["--probes", "/nonexistent/probes.txt"], "cannot open probe file /nonexistent/probes.txt"),
    (["--probe-line", "0", "0", "1", "1", "65536", "--probe-line", "5", "5", "5", "5", "1"], "65537 points, at most 65536")])
def test_bad_probe_options_are_refused_with_the_reason(probes_check, args, message):
    r = probes_check(128, 32, *args)
    assert r.returncode == 2 and message in r.stderr, (r.returncode, r.stderr)


# ---- lbm_solver --probes / --probe-line ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    subprocess.check_call(["make", "-s", "-C", HOST])
    exe = os.path.join(HOST, "lbm_solver")
    assert os.path.exists(exe), "host/lbm_solver was not built"
    return exe


def test_help_documents_both_flags(solver):
    r = subprocess.run([solver, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--probes FILE" in r.stdout and "--probe-line x0 y0 x1 y1 n" in r.stdout and "probes.csv" in r.stdout


@pytest.mark.parametrize("args, message", [
    (["--probe-line", "40", "2", "40", "32", "10"], "probe 9: (40, 32) outside the domain 0..127 x 0..31"),
    (["--probe-line", "40", "2", "40"], "--probe-line takes five values"),
    (["--probes"], "missing value for --probes"),
    (["--probes", "no_such_file.txt"], "cannot open probe file no_such_file.txt"),
    (["--probe-line", "40", "2", "40", "29", "10", "--output-frequency", "0"], "need --output-frequency > 0")])
def test_lbm_solver_refuses_bad_probes_before_opening_a_device(solver, tmp_path, args, message):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")
    r = subprocess.run([solver, "--nx", "128", "--ny", "32", "--steps", "10", "--output-frequency", "5"] + args, cwd=tmp_path, capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert message in r.stderr and "unknown option" not in r.stderr, r.stderr
    assert "MI355X HIP Grid" not in r.stdout
    assert os.listdir(tmp_path) == []


def test_lbm_solver_accepts_valid_probes(solver, tmp_path):
    """Positive control: without a device the run ends at the first device call (exit code 1); with one it completes."""
    (tmp_path / "p.txt").write_text(PROBE_FILE)
    r = subprocess.run([solver, "--nx", "128", "--ny", "32", "--steps", "11", "--output-frequency", "5", "--probes", "p.txt", "--probe-line", "40", "2",
                        "40", "29", "10", "--no-vtk", "--no-tune", "--quiet"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)
    assert "probe" not in r.stderr and "unknown option" not in r.stderr, r.stderr
    if r.returncode == 0:
        rows = (tmp_path / "probes.csv").read_text().splitlines()
        assert rows[0] == "timestep,probe,x,y,rho,ux,uy" and len(rows) == 1 + 3 * 14
