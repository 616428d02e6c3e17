"""Per-body momentum-exchange forces (lbm_set_body_labels / k_forces_bodies), the part that needs no GPU: the exported symbols, the
partition lbm_set_body_labels derives from a label array (lbm_debug_body_chunks against numpy), the place of the per-body sample in
the launch choreography (option bodies=1 of lbm_debug_choreography) and the command line of lbm_solver --obstacle-bodies.

A label array is the global [ny][nx] byte array of lbm_set_solid_mask read as body numbers (0 fluid, k = 1..255 a cell of body k; B = the
largest label present). For one strip the host keeps, per body, its bounding box dilated by one cell and clipped to the domain and to
the strip's rows, and cuts every non-empty box into chunks of FORCE_CHUNK = 65536 cells: one block of the kernel per chunk, partial
sums added per body in chunk order. lbm_create needs a device, so the argument checks of lbm_set_body_labels on a context live in
tests/test_gpu_bodies.py."""
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
from tests.helpers import PKG, STAT_CALLS, geometries, ops_of, sample_points, write_pgm

SYMBOLS = ("lbm_set_body_labels", "lbm_body_count", "lbm_get_body_forces", "lbm_drain_body_force_log", "lbm_debug_body_chunks")
LBM_ERR_ARG = -1
FORCE_CHUNK = 65536


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    return pkg


@pytest.fixture(scope="module")
def L(lbm):
    lib = C.CDLL(lbm.lib_path())
    for s in SYMBOLS:          # (AttributeError on a library without per-body forces)
        getattr(lib, s)
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
    L.lbm_set_body_labels.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
    L.lbm_get_body_forces.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.lbm_drain_body_force_log.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.lbm_body_count.argtypes = [C.c_void_p]
    lab = (C.c_ubyte * 4)()
    assert L.lbm_set_body_labels(None, lab, 2, 2) == LBM_ERR_ARG
    assert L.lbm_body_count(None) == 0
    assert L.lbm_get_body_forces(None, (C.c_double * 2)()) == LBM_ERR_ARG
    assert L.lbm_drain_body_force_log(None, None, 0) == LBM_ERR_ARG


# ---- the partition: lbm_debug_body_chunks against numpy --------------------------------------------------------------------
def expected(labels, y_start, local_ny):
    """B, boxes [B, 4] (x0, x1, y0, y1 inclusive, local y; {0, -1, 0, -1} where empty), chunks [(body, first, cells)]."""
    ny, nx = labels.shape
    B = int(labels.max())
    boxes, chunks = [], []
    for k in range(1, B + 1):
        ys, xs = np.nonzero(labels == k)
        box = (0, -1, 0, -1)
        if len(ys):
            x0, x1 = max(0, xs.min() - 1), min(nx - 1, xs.max() + 1)
            y0, y1 = max(0, ys.min() - 1 - y_start), min(local_ny - 1, ys.max() + 1 - y_start)
            if y1 >= y0:
                box = (int(x0), int(x1), int(y0), int(y1))
        boxes.append(box)
        cells = (box[1] - box[0] + 1) * (box[3] - box[2] + 1) if box[1] >= box[0] else 0
        chunks += [(k, f, min(FORCE_CHUNK, cells - f)) for f in range(0, cells, FORCE_CHUNK)]
    return B, np.array(boxes, dtype=np.int32).reshape(B, 4), np.array(chunks, dtype=np.int64).reshape(len(chunks), 3)


def check(lbm, labels, y_start, local_ny):
    B, boxes, chunks = lbm.debug_body_chunks(labels, y_start, local_ny)
    eB, eboxes, echunks = expected(labels, y_start, local_ny)
    assert B == eB
    assert np.array_equal(boxes, eboxes), (boxes, eboxes)
    assert np.array_equal(chunks, echunks), (chunks, echunks)
    return B, boxes, chunks


def tandem(nx=192, ny=64, second=2):
    y, x = np.mgrid[0:ny, 0:nx]
    lab = np.zeros((ny, nx), np.uint8)
    lab[(x - 50) ** 2 + (y - ny // 2) ** 2 <= 36] = 1
    lab[(x - 90) ** 2 + (y - ny // 2) ** 2 <= 36] = second
    return lab


def walls(nx=192, ny=64):
    lab = np.zeros((ny, nx), np.uint8)
    lab[0:10, 100:116] = 1
    lab[20:30, 0:1] = 2
    lab[40:50, nx - 1:nx] = 3
    return lab


@pytest.mark.parametrize("bounds", [[(0, 64)], [(0, 22), (22, 21), (43, 21)]])
def test_boxes_and_chunks_of_a_whole_domain_and_of_three_strips(lbm, bounds):
    for lab in (tandem(), walls()):
        for y0, n in bounds:
            check(lbm, lab, y0, n)
    # the whole-domain boxes, spelled out: a disc of radius 6 around (50, 32) and its dilation; bodies on the walls are clipped
    if len(bounds) == 1:
        _, boxes, chunks = lbm.debug_body_chunks(tandem())
        assert boxes.tolist() == [[43, 57, 25, 39], [83, 97, 25, 39]] and chunks.tolist() == [[1, 0, 225], [2, 0, 225]]
        _, boxes, _ = lbm.debug_body_chunks(walls())
        assert boxes.tolist() == [[99, 116, 0, 10], [0, 1, 19, 30], [190, 191, 39, 50]]


def test_a_body_on_a_strip_boundary_and_a_body_outside_the_strip(lbm):
    lab = tandem()      # rows 26..38
    # the strip boundary at row 32 runs through both discs: each strip holds its part of the dilated box
    _, lo, _ = check(lbm, lab, 0, 32)
    _, hi, _ = check(lbm, lab, 32, 32)
    assert lo[0].tolist() == [43, 57, 25, 31] and hi[0].tolist() == [43, 57, 0, 7]
    # a strip that ends directly below the box's first row (25) holds nothing of it; one row more holds one row of it
    B, boxes, chunks = check(lbm, lab, 0, 25)
    assert B == 2 and boxes.tolist() == [[0, -1, 0, -1]] * 2 and len(chunks) == 0
    _, boxes, chunks = check(lbm, lab, 0, 26)
    assert boxes[0].tolist() == [43, 57, 25, 25] and chunks.tolist() == [[1, 0, 15], [2, 0, 15]]
    # ... and the same above it (last row of the dilated box: 39)
    _, boxes, chunks = check(lbm, lab, 40, 24)
    assert boxes.tolist() == [[0, -1, 0, -1]] * 2 and len(chunks) == 0
    _, boxes, _ = check(lbm, lab, 39, 25)
    assert boxes[1].tolist() == [83, 97, 0, 0]
    # the walls set: body 1 (rows 0..9) is outside the top strip, body 3 (rows 40..49) outside the bottom strip
    B, boxes, chunks = check(lbm, walls(), 43, 21)
    assert B == 3 and boxes[0].tolist() == [0, -1, 0, -1] and sorted(set(chunks[:, 0].tolist())) == [3]


def test_a_label_gap_is_a_body_without_chunks(lbm):
    B, boxes, chunks = check(lbm, tandem(second=3), 0, 64)
    assert B == 3 and boxes[1].tolist() == [0, -1, 0, -1] and chunks[:, 0].tolist() == [1, 3]
    # the largest label alone decides B
    lab = np.zeros((16, 16), np.uint8); lab[8, 8] = 255
    B, boxes, chunks = check(lbm, lab, 0, 16)
    assert B == 255 and chunks.tolist() == [[255, 0, 9]] and boxes[254].tolist() == [7, 9, 7, 9]
    # no label at all: no body
    B, boxes, chunks = lbm.debug_body_chunks(np.zeros((16, 16), np.uint8))
    assert B == 0 and len(boxes) == 0 and len(chunks) == 0


def test_a_box_of_more_than_one_chunk(lbm):
    nx, ny = 512, 160
    y, x = np.mgrid[0:ny, 0:nx]
    lab = np.zeros((ny, nx), np.uint8)
    lab[(x % 16 == 8) & (y % 16 == 8)] = 1
    lab[(x - 100) ** 2 + (y - 80) ** 2 <= 64] = 2
    B, boxes, chunks = check(lbm, lab, 0, ny)
    assert boxes[0].tolist() == [7, 505, 7, 153]      # posts at 8..504 x 8..152, dilated: 499 x 147 cells
    assert chunks[chunks[:, 0] == 1].tolist() == [[1, 0, 65536], [1, 65536, 499 * 147 - 65536]]
    assert chunks[chunks[:, 0] == 2].tolist() == [[2, 0, 19 * 19]]
    # exactly one chunk, and one cell more
    lab = np.zeros((258, 258), np.uint8); lab[1:255, 1:255] = 1      # box 256 x 256 = 65536
    assert check(lbm, lab, 0, 258)[2].tolist() == [[1, 0, 65536]]
    lab[1:255, 255] = 1                                              # box 257 x 256
    assert check(lbm, lab, 0, 258)[2].tolist() == [[1, 0, 65536], [1, 65536, 256]]
    # three strips of the posts: every strip's chunks follow from its own clipped box
    for y0, n in [(0, 54), (54, 53), (107, 53)]:
        check(lbm, np.where((x % 16 == 8) & (y % 16 == 8), 1, 0).astype(np.uint8), y0, n)


def test_bad_arguments_of_the_hook(L):
    L.lbm_debug_body_chunks.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_long),
                                        C.c_int, C.POINTER(C.c_int)]
    lab = (C.c_ubyte * 16)()
    assert L.lbm_debug_body_chunks(None, 4, 4, 0, 4, None, 0, None, 0, None) == LBM_ERR_ARG
    assert L.lbm_debug_body_chunks(lab, 4, 4, 2, 3, None, 0, None, 0, None) == LBM_ERR_ARG      # strip beyond the domain
    lab[5] = 2
    assert L.lbm_debug_body_chunks(lab, 4, 4, 0, 4, (C.c_int * 4)(), 1, None, 0, None) == LBM_ERR_ARG      # two bodies, room for one box


def test_labels_outside_a_byte_are_refused_by_the_binding(lbm):
    with pytest.raises(ValueError):
        lbm.debug_body_chunks(np.full((4, 4), 256, np.int32))
    with pytest.raises(TypeError):
        lbm.debug_body_chunks(np.zeros((4, 4), np.float64))


# ---- the choreography: the per-body sample sits directly behind the force kernel, in every schedule -------------------------
def test_the_body_sample_is_ordered_and_fresh_in_every_schedule(dry):
    """bodies=1: 0 violations (no RACE, no STALE) for transports 0-3, every overlap x deep_halo schedule and every plan family of
    tests/test_stats_cpu.py; one "body forces" operation per strip and force point, directly behind the force kernel of that strip and
    iteration, reading the rows the force kernel reads; without the option the record is that of a run without labels."""
    runs = 0
    for (plan, prec), dh, ov in itertools.product(tc.PLANS, (0, 1, 2), (0, 1, 2)):
        opts = dict(tune=0, nt=1, xcd=1, overlap=ov, deep_halo=dh, trailing_pair=0, **plan)
        for transport, bounds, ny in geometries():
            for calls in STAT_CALLS:
                rc, text = dry(256, ny, bounds, transport, dict(opts, bodies=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} bodies=1 transport {transport} bounds {bounds} calls {calls}: rc {rc}\n{text[:3000]}"
                forces, bodies = ops_of(text, "forces"), ops_of(text, "body forces")
                for k in range(len(bounds)):
                    assert [t for s, t in bodies if s == k] == [t for s, t in forces if s == k] == sample_points(calls, 0)
                lines = text.splitlines()
                for i, ln in enumerate(lines):
                    if ": body forces t=" in ln:
                        assert ": forces t=" in lines[i - 1], lines[i - 1:i + 1]
                        assert ln.split(": body forces ")[1].replace(", writes its log slot", "") == lines[i - 1].split(": forces ")[1]
                        assert ln.split(" main")[0].split(" ", 1)[1] == lines[i - 1].split(" main")[0].split(" ", 1)[1]
                rc0, plain = dry(256, ny, bounds, transport, opts, calls, prec, dump=1)
                strip_no = lambda s: [re.sub(r"^#\d+ ", "", ln) for ln in s.splitlines() if ": body forces t=" not in ln]
                assert rc0 == 0 and ": body forces" not in plain and strip_no(text) == strip_no(plain)
    assert runs > 2500


def test_the_body_sample_beside_the_statistics_sample(dry):
    """Both options: forces, body forces, stats, in this order, no violation."""
    b, ny = tc.strips_of((13, 24, 17))
    rc, text = dry(256, ny, b, 0, dict(tune=0, nt=1, xcd=1, overlap=1, deep_halo=1, deep=7, arith=1, stats=0, bodies=1), [(31, 7)], dump=1)
    assert rc == 0, text
    kinds = [ln.split(" stream: ")[1].split(" t=")[0] for ln in text.splitlines() if "strip 1 main stream" in ln and " t=7 reads" in ln]
    assert kinds == ["forces", "body forces", "stats"], kinds


def test_the_body_sample_needs_no_ghost_row(dry):
    """With the exchange cut ("skip_exchange") the statistics sample of a middle rank is STALE: it reads one ghost row per face. The body
    sample beside it reads the strip's own rows only, like the force kernel, and is not named."""
    rc, text = dry(256, 384, [(128, 128)], 2, dict(tune=0, nt=1, xcd=1, overlap=0, deep_halo=0, fuse=1, skip_exchange=1, stats=0, bodies=1), [(3, 2)])
    assert rc > 0 and "stats t=2" in text and "body forces t=2" not in text, text


def test_split_plans_take_the_body_sample_on_the_joined_main_stream(dry):
    runs = 0
    for (plan, prec), sp, smin in itertools.product(ts.PLANS, (3, 4), (1, 8)):
        opts = dict(tune=0, nt=0, xcd=1, alternate=1, trailing_pair=0, split=sp, split_min=smin, **plan)
        for ny in (24, 64, 133, 256, 1024):
            for calls in ([(31, 7)], [(97, 31), (5, 0)], [(5, 0), (20, 0), (97, 10)], [(120, 30)]):
                rc, text = dry(256, ny, [(0, ny)], 0, dict(opts, bodies=1), calls, prec, dump=1)
                runs += 1
                assert rc == 0, f"{opts} ny {ny} calls {calls}: rc {rc}\n{text[:3000]}"
                assert [t for _, t in ops_of(text, "body forces")] == sample_points(calls, 0)
    assert runs > 300


# ---- lbm_solver --obstacle-bodies -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(lbm):
    exe = os.path.join(os.path.dirname(lbm.__file__), "host", "lbm_solver")
    assert os.path.exists(exe), "host/lbm_solver was not built"
    return exe


def test_lbm_solver_refuses_bodies_together_with_a_mask(solver, tmp_path):
    out = tmp_path / "run"; out.mkdir()
    write_pgm(tmp_path / "b.pgm", tandem(64, 32))
    r = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10", "--obstacle-bodies", str(tmp_path / "b.pgm"), "--obstacle-mask",
                        str(tmp_path / "b.pgm")], cwd=out, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "--obstacle-bodies" in r.stderr and "--obstacle-mask" in r.stderr and "unknown option" not in r.stderr, r.stderr
    assert os.listdir(out) == []


@pytest.mark.parametrize("shape, maxval, message", [((32, 60), 255, "image is 60x32, the lattice 64x32"), ((32, 64), 65535, "maxval 65535")])
def test_lbm_solver_refuses_a_bad_bodies_file_before_opening_a_device(solver, tmp_path, shape, maxval, message):
    out = tmp_path / "run"; out.mkdir()
    lab = np.zeros(shape, np.uint8); lab[10:20, 10:20] = 1; lab[10:20, 30:40] = 2
    write_pgm(tmp_path / "b.pgm", lab, maxval)
    r = subprocess.run([solver, "--nx", "64", "--ny", "32", "--steps", "10", "--obstacle-bodies", str(tmp_path / "b.pgm")], cwd=out,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "--obstacle-bodies" in r.stderr and message in r.stderr and "unknown option" not in r.stderr, r.stderr
    assert os.listdir(out) == []


def test_lbm_solver_accepts_a_valid_bodies_file(solver, tmp_path):
    """Positive control: a well-formed file passes the command line. Without a device the run ends at the first device call (exit code
    1); with one it completes and writes forces_bodies.csv. Either way it is not the exit code 2 of a refused option."""
    write_pgm(tmp_path / "b.pgm", tandem(128, 48))
    out = tmp_path / "run"; out.mkdir()
    r = subprocess.run([solver, "--nx", "128", "--ny", "48", "--steps", "10", "--output-frequency", "5", "--obstacle-bodies", str(tmp_path / "b.pgm"),
                        "--no-vtk", "--no-tune", "--quiet"], cwd=out, capture_output=True, text=True, timeout=60)
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)
    assert "unknown option" not in r.stderr, r.stderr
    if r.returncode == 0:
        assert os.path.exists(out / "forces_bodies.csv")
