"""The per-wave verdict of the register kernel (csrc/lbm_kernels.hpp wave_plain, through lbm_debug_wave_plain: the very function the
kernel's branch calls, compiled for the host) without a GPU.

A block of k_stepc_col that is not lean as a whole (a wall tile, a partial band, a strip's edge) still sends down the lean path every
wave whose rows are plain interior fluid at every level. The verdict is held against a brute-force classification written here, cell by
cell and level by level from the tests the general path makes (csrc/lbm_kernel_col.hpp):
  level 1       a cell must exist (a column, a row of the lattice the kernel counts), be loaded (y <= y_end + HW - 1), be no cell of
                column 0 or nx - 1 (ports, inlet profile) or of row 0 or ny_glob - 1 (walls of any kind), and not be solid
  levels 2..D   a cell inside the level's window must be counted by the general path (y <= y_end + HW - L), since the lean path counts it
  level D       a cell the lean path stores (the middle OW x OH cells) must be one the general path stores (y < y_end)
A periodic lattice is the strip PERIODIC_PAD = 16 rows up in a lattice of ny + 32 rows with the geometry wrapped, as the kernels see it.
plain => brute-force plain always; the converse wherever the block-uniform near-solid test (conservative by 8x8 blocks, or by the
disc's bounding box) says no solid cell is near, which is where every other term of the verdict is exact."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from tests.helpers import PKG, deep_shapes

PAD = 16
F64, F32 = 0, 1
# (deep id, iterations of the launch, precision, arith): every depth of every region kind, both fp64 shapes of 64x32, both fp32 tall shapes
KINDS = [(6, 5, F64, 1), (7, 6, F64, 1), (9, 7, F64, 1), (7, 6, F64, 0), (9, 7, F64, 0), (7, 6, F32, 1), (9, 7, F32, 0),
         (10, 5, F64, 1), (10, 6, F64, 1), (11, 7, F64, 1), (8, 6, F32, 1), (8, 7, F32, 1), (8, 8, F32, 0)]


@functools.lru_cache(maxsize=None)
def library():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    L = C.CDLL(pkg.lib_path())
    L.lbm_debug_wave_plain.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_ubyte), C.POINTER(C.c_double)] + [C.c_int] * 7 + [C.POINTER(C.c_int)]
    L.lbm_debug_wave_plain.restype = C.c_int
    L.lbm_last_error.restype = C.c_char_p
    return L


def verdict(nx, ny, y_start, local_ny, precision, arith, periodic, mask, deep, depth, y_lo, y_cnt, bx, by, wave, cyl=None):
    L = library()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).ctypes.data_as(C.POINTER(C.c_ubyte))
    c3 = None if cyl is None else (C.c_double * 3)(*cyl)
    dims = (C.c_int * 4)()
    rc = L.lbm_debug_wave_plain(nx, ny, y_start, local_ny, precision, arith, int(periodic), m, c3, deep, depth, y_lo, y_cnt, bx, by, wave, dims)
    assert rc in (0, 1), L.lbm_last_error()
    return rc, tuple(dims)


def rows_waves(deep, precision, arith):
    r = deep_shapes()[deep, "f32" if precision == F32 else "f64", arith]
    return r.rows, r.waves


def solid_field(nx, ny, mask, cyl):
    if mask is not None:
        return np.asarray(mask, bool)
    cx, cy, r = int(cyl[0] * nx), int(cyl[1] * ny), int(cyl[2] * ny)
    y, x = np.mgrid[0:ny, 0:nx]
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def brute(nx, ny, y_start, periodic, solid, R, NW, D, y_lo, y_cnt, bx, by, wave):
    """(plain, any solid cell in the tile's region) of one wave, cell by cell and level by level."""
    H, HW = R * NW, D - 1
    OW, OH = 64 - 2 * HW, H - 2 * HW
    ny_glob, ys = (ny + 2 * PAD, y_start + PAD) if periodic else (ny, y_start)
    y_end, Xo, Yo = y_lo + y_cnt, bx * OW, y_lo + by * OH

    def is_solid(x, yg):                  # (arrays of cells: one answer per cell)
        inside = (x >= 0) & (x < nx) & (np.full(yg.shape, True) if periodic else (yg >= 0) & (yg < ny))
        rows = (yg - PAD) % ny if periodic else np.clip(yg, 0, ny - 1)
        return inside & solid[rows, np.clip(x, 0, nx - 1)]
    ry_all, lane_all = np.mgrid[0:H, 0:64]
    region_solid = bool(is_solid(Xo - HW + lane_all, ys + Yo - HW + ry_all).any())
    ry, lane = np.mgrid[wave * R:(wave + 1) * R, 0:64]          # one entry per cell of the wave
    x, y = Xo - HW + lane, Yo - HW + ry
    yg = ys + y
    ok = (x >= 0) & (x < nx) & (yg >= 0) & (yg < ny_glob)                          # the cell exists
    ok &= y <= y_end + HW - 1                                                      # level 1 loads it
    ok &= (x != 0) & (x != nx - 1) & (yg != 0) & (yg != ny_glob - 1)               # no port, no wall
    ok &= ~is_solid(x, yg)
    for lvl in range(2, D + 1):
        window = (ry >= lvl - 1) & (ry <= H - lvl) & (lane >= lvl - 1) & (lane <= 64 - lvl)
        ok &= ~window | (y <= y_end + HW - lvl)                                    # counted by both paths
    stored = (ry >= HW) & (ry < H - HW) & (lane >= HW) & (lane < 64 - HW)
    ok &= ~stored | (y < y_end)                                                    # stored by both paths
    return bool(ok.all()), region_solid


def check_launch(nx, ny, y_start, local_ny, periodic, mask, kind, y_lo, y_cnt, cyl=(0.2, 0.5, 0.05), columns=None):
    deep, depth, precision, arith = kind
    R, NW = rows_waves(deep, precision, arith)
    HW = depth - 1
    OW, OH = 64 - 2 * HW, R * NW - 2 * HW
    cnt = y_cnt if y_cnt > 0 else local_ny
    lo = y_lo if y_cnt > 0 else 0
    solid = solid_field(nx, ny, mask, cyl)
    nbx, nby = -(-nx // OW), -(-cnt // OH)
    seen = 0
    for by in range(nby):
        for bx in (columns if columns is not None else range(nbx)):
            for w in range(NW):
                got, dims = verdict(nx, ny, y_start, local_ny, precision, arith, periodic, mask, deep, depth, y_lo, y_cnt, bx, by, w, cyl)
                assert dims[:2] == (R, NW)
                want, region_solid = brute(nx, ny, y_start, periodic, solid, R, NW, depth, lo, cnt, bx, by, w)
                where = (nx, ny, y_start, local_ny, periodic, kind, y_lo, y_cnt, bx, by, w)
                assert not (region_solid and not dims[3]), ("a solid cell in a tile that is not near_solid", where)
                assert not (got and not want), ("plain, but a cell of the wave is not", where)
                if not dims[3]:
                    assert got == int(want), ("every cell of the wave is plain, the verdict is not", where)
                if dims[2]:
                    assert want, ("a lean block with a wave that is not plain", where)
                seen += got
    return seen


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: "deep%d-%dit-%s-%s" % (k[0], k[1], "f32" if k[2] else "f64", "contracted" if k[3] else "strict"))
def test_whole_domains(kind):
    """Walled domains whose wall rows land on every row index of a wave: 57..62 rows and 90 rows; no solid cell near (the disc is tiny)."""
    far = (0.99, 0.0, 0.0)          # (a one-cell disc in the last column of row 0, where the walls and the outlet bar every wave anyway)
    total = 0
    for ny in (57, 58, 59, 60, 61, 62):
        total += check_launch(170, ny, 0, ny, False, None, kind, 0, 0, cyl=far)
    total += check_launch(230, 90, 0, 90, False, None, kind, 0, 0)          # (the default disc: its box bars the tiles it touches)
    assert total > 0


@pytest.mark.parametrize("kind", [(7, 6, F64, 1), (11, 7, F64, 1), (9, 7, F64, 0), (8, 7, F32, 1)], ids=lambda k: "deep%d-%dit" % k[:2])
def test_ranges_strips_periodic_and_masks(kind):
    nx = 170
    cell = np.zeros((90, nx), np.uint8)
    cell[1, 80] = 1                                   # one solid cell next to the bottom wall inside a middle tile column
    top = np.zeros((90, nx), np.uint8)
    top[88, 60] = 1
    # range launches of a whole domain (option "split": the last range holds the partial band) and arbitrary cuts
    for y_lo, y_cnt in ((0, 30), (30, 30), (60, 30), (0, 44), (44, 46), (7, 61)):
        check_launch(nx, 90, 0, 90, False, None, kind, y_lo, y_cnt, cyl=(0.99, 0.0, 0.0))
    # a group of two strips: whole-strip launches, edge bands and the middle of a strip with a face
    for y_start, rows in ((0, 45), (45, 45), (0, 31), (31, 59)):
        for y_lo, y_cnt in ((0, 0), (0, 6), (rows - 6, 6), (6, rows - 12)):
            check_launch(nx, 90, y_start, rows, False, None, kind, y_lo, y_cnt, cyl=(0.99, 0.0, 0.0))
    # periodic y: no wall row anywhere; the wrapped geometry is a mask (the disc rasterised, or the user's)
    check_launch(nx, 90, 0, 90, True, None, kind, 0, 0, cyl=(0.99, 0.0, 0.0))
    check_launch(nx, 90, 0, 90, True, cell, kind, 0, 0)
    check_launch(nx, 90, 0, 45, True, None, kind, 0, 0)
    # a one-cell mask next to either wall: the tile is near a solid cell, none of its waves is plain
    for m in (cell, top):
        check_launch(nx, 90, 0, 90, False, m, kind, 0, 0)
    OW = 64 - 2 * (kind[1] - 1)
    R, NW = rows_waves(kind[0], kind[2], kind[3])
    assert all(verdict(nx, 90, 0, 90, kind[2], kind[3], False, cell, kind[0], kind[1], 0, 0, 80 // OW, 0, w)[0] == 0 for w in range(NW))


def test_headline_counts():
    """4096x1024 fp64 contracted at seven iterations on 64x40 regions (79 x 37 tiles): four plain waves in each top wall tile of a middle
    column, six in each bottom one; no wave of tile columns 0 and 78; a lean block needs no verdict (every wave of it is plain)."""
    nx, ny, kind = 4096, 1024, (11, 7, F64, 1)
    far = (0.2, 0.5, 0.05)
    for bx in (1, 2, 40, 77):
        top = [verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 0, 0, bx, 36, w, far) for w in range(8)]
        bottom = [verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 0, 0, bx, 0, w, far) for w in range(8)]
        assert [v for v, _ in top] == [1, 1, 1, 1, 0, 0, 0, 0] and [v for v, _ in bottom] == [0, 0, 1, 1, 1, 1, 1, 1], (bx, top, bottom)
        assert all(d == (5, 8, 0, 0) for _, d in top + bottom)
    for bx in (0, 78):
        assert sum(verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 0, 0, bx, by, w, far)[0] for by in (0, 1, 36) for w in range(8)) == 0
    mid = [verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 0, 0, 40, 1, w, far) for w in range(8)]
    assert all(v == 1 and d[2] == 1 for v, d in mid)
    # the same launch as three ranges (option "split" 3 cuts at band boundaries): the wall tiles keep their counts
    OH = 28
    assert sum(verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 24 * OH, ny - 24 * OH, 40, 12, w, far)[0] for w in range(8)) == 4
    assert sum(verdict(nx, ny, 0, ny, F64, 1, False, None, 11, 7, 0, 12 * OH, 40, 0, w, far)[0] for w in range(8)) == 6
    # brute force on one middle column of the headline grid
    assert check_launch(nx, ny, 0, ny, False, None, kind, 0, 0, columns=(40,)) == 4 + 6 + 35 * 8


def test_large_buffers_and_arguments():
    """A buffer of 4 GiB or more has no lean path (32-bit byte offsets), hence no plain wave; the argument errors."""
    assert sum(verdict(16384, 4200, 0, 4200, F64, 1, False, None, 11, 7, 0, 0, 5, by, w)[0] for by in (0, 1, 149) for w in range(8)) == 0
    assert sum(verdict(16384, 2000, 0, 2000, F64, 1, False, None, 11, 7, 0, 0, 5, 1, w)[0] for w in range(8)) == 8
    L = library()
    bad = [dict(nx=0), dict(local_ny=91), dict(precision=2), dict(arith=2), dict(periodic=2), dict(deep=1), dict(deep=8), dict(depth=8),
           dict(bx=4), dict(by=5), dict(wave=8), dict(wave=-1)]
    for b in bad:
        a = dict(nx=170, ny=90, y_start=0, local_ny=90, precision=F64, arith=1, periodic=0, deep=7, depth=6, y_lo=0, y_cnt=0, bx=1, by=1, wave=0)
        a.update(b)
        rc = L.lbm_debug_wave_plain(a["nx"], a["ny"], a["y_start"], a["local_ny"], a["precision"], a["arith"], a["periodic"], None, None,
                                    a["deep"], a["depth"], a["y_lo"], a["y_cnt"], a["bx"], a["by"], a["wave"], None)
        assert rc == -1 and b"lbm_debug_wave_plain" in L.lbm_last_error(), (b, rc, L.lbm_last_error())
