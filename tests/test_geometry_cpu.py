"""User-defined obstacle geometry, the parts that need no GPU: lbm_solver's PGM checks (a bad --obstacle-mask file is refused before
any device is touched) and the host-side packing lbm_set_solid_mask hands to the kernels (lbm_debug_geometry): the window bitmap of a
strip and the coarse summed-area table behind the kernels' block-uniform near-solid query, against numpy."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import lbm_cpu, solver  # noqa: F401
GR = 12   # ghost rows a strip's window reaches beyond its own rows (csrc/lbm_kernels.hpp GR)


def run_solver(solver, cwd, pgm, nx=16, ny=8):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")   # (a device opened anyway would fail differently: "lbm_create" / "no HIP device")
    return subprocess.run([solver, "--nx", str(nx), "--ny", str(ny), "--steps", "1", "--no-vtk", "--obstacle-mask", str(pgm)],
                          cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60, env=env)


@pytest.mark.parametrize("name,data,why", [
    ("magic", b"P6\n16 8\n255\n" + bytes(16 * 8 * 3), "not a PGM"),
    ("header", b"P5\n16 x\n255\n" + bytes(128), "bad PGM header"),
    ("size", b"P5\n16 9\n255\n" + bytes(16 * 9), "the lattice 16x8"),
    ("short", b"P5\n16 8\n255\n" + bytes(100), "short pixel data"),
    ("maxval", b"P5\n16 8\n65535\n" + bytes(256), "maxval 65535"),
    ("ascii-short", b"P2\n16 8\n1\n" + b"0 " * 100, "short or bad pixel data"),
    ("ascii-range", b"P2\n16 8\n1\n" + b"2 " * 128, "above maxval"),
    ("empty", b"P5\n16 8\n255\n" + bytes(128), "no solid pixel"),
])
def test_malformed_pgm_is_refused_before_any_device(solver, tmp_path, name, data, why):
    p = tmp_path / f"{name}.pgm"
    p.write_bytes(data)
    pr = run_solver(solver, tmp_path, p)
    assert pr.returncode != 0
    assert why in pr.stderr, pr.stderr
    assert "lbm_create" not in pr.stderr and "HIP" not in pr.stderr and "MI355X HIP Grid" not in pr.stdout


def test_missing_pgm_is_refused(solver, tmp_path):
    pr = run_solver(solver, tmp_path, tmp_path / "nope.pgm")
    assert pr.returncode != 0 and "cannot open obstacle mask" in pr.stderr


def bits_of(mask, y0, rows):
    ny, nx = mask.shape
    words = (nx + 63) // 64
    padded = np.zeros((rows, words * 64), dtype=np.uint64)
    padded[:, :nx] = mask[y0:y0 + rows] != 0
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(rows, words, 64) * weights).sum(axis=2, dtype=np.uint64)


@pytest.mark.parametrize("seed", range(6))
def test_packing_and_near_query_against_numpy(lbm, seed):
    rng = np.random.default_rng(seed)
    nx, ny = int(rng.integers(1, 300)), int(rng.integers(1, 120))
    density = [0.0, 0.002, 0.05, 0.5][seed % 4]
    mask = (rng.random((ny, nx)) < density).astype(np.uint8)
    if seed == 5:
        mask[:] = 0
        mask[ny - 1, nx - 1] = 1                     # one cell in the last (ragged) column and row
    y_start = int(rng.integers(0, ny))
    local_ny = int(rng.integers(1, ny - y_start + 1))
    boxes = []
    for _ in range(400):
        x0, y0 = int(rng.integers(-20, nx + 20)), int(rng.integers(-20, ny + 20))
        boxes.append((x0, x0 + int(rng.integers(0, 70)), y0, y0 + int(rng.integers(0, 40))))
    d, bits, sat, near = lbm.debug_geometry(mask * np.uint8(1 + seed), y_start, local_ny, boxes)   # (any nonzero byte is solid)
    wy0, wy1 = max(0, y_start - GR), min(ny, y_start + local_ny + GR)
    assert (d["y0"], d["rows"], d["words"], d["nbx"], d["nby"]) == (wy0, wy1 - wy0, (nx + 63) // 64, (nx + 7) // 8, (wy1 - wy0 + 7) // 8)
    assert np.array_equal(bits, bits_of(mask, wy0, wy1 - wy0))
    ys, xs = np.nonzero(mask)
    if len(xs):
        assert (d["bx0"], d["bx1"], d["by0"], d["by1"]) == (xs.min(), xs.max(), ys.min(), ys.max())
    else:
        assert d["bx1"] < d["bx0"]
    # the coarse table: solid counts of the 8x8 blocks of the window, summed
    win = np.zeros((d["nby"] * 8, d["nbx"] * 8), dtype=np.int64)
    win[:wy1 - wy0, :nx] = mask[wy0:wy1]
    blocks = win.reshape(d["nby"], 8, d["nbx"], 8).sum(axis=(1, 3))
    ref = np.zeros((d["nby"] + 1, d["nbx"] + 1), dtype=np.int64)
    ref[1:, 1:] = blocks.cumsum(0).cumsum(1)
    assert np.array_equal(sat, ref)
    # the near query: never misses a solid cell of the window, and is exact at block granularity
    for (x0, x1, y0, y1), got in zip(boxes, near):
        cx0, cx1, cy0, cy1 = max(x0, 0), min(x1, nx - 1), max(y0, wy0), min(y1, wy1 - 1)
        exact = cx0 <= cx1 and cy0 <= cy1 and bool(mask[cy0:cy1 + 1, cx0:cx1 + 1].any())
        kx1 = min(x1, d["nbx"] * 8 - 1)             # (columns clip to the last whole block: nothing is solid beyond nx)
        bx0, bx1, by0, by1 = cx0 // 8 * 8, kx1 // 8 * 8 + 7, (cy0 - wy0) // 8 * 8 + wy0, (cy1 - wy0) // 8 * 8 + 7 + wy0
        coarse = cx0 <= kx1 and cy0 <= cy1 and bool(mask[max(by0, wy0):min(by1, wy1 - 1) + 1, bx0:bx1 + 1].any())
        assert not exact or got, (x0, x1, y0, y1)
        assert bool(got) == coarse, (x0, x1, y0, y1)


def test_debug_geometry_arguments(lbm):
    import ctypes as C
    L = lbm.lib()
    dims = (C.c_int * 9)()
    m = np.zeros((8, 16), np.uint8)
    ub = C.POINTER(C.c_ubyte)
    assert L.lbm_debug_geometry(None, 16, 8, 0, 8, dims, None, 0, None, 0, None, 0, None) == -1
    assert L.lbm_debug_geometry(m.ctypes.data_as(ub), 16, 8, 4, 8, dims, None, 0, None, 0, None, 0, None) == -1   # strip beyond ny
    assert L.lbm_debug_geometry(m.ctypes.data_as(ub), 16, 8, 0, 8, dims, None, 0, None, 0, None, 0, None) == 0
    bits = (C.c_ulonglong * 1)()
    assert L.lbm_debug_geometry(m.ctypes.data_as(ub), 16, 8, 0, 8, dims, bits, 0, None, 0, None, 0, None) == -1   # too small
    with pytest.raises(ValueError):
        lbm.debug_geometry(np.zeros((3, 4, 5)))
