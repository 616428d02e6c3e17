"""One-cell obstacles swept, position by position, across tile edges, strip faces, walls and corners.

Every fused kernel decides once per block whether a cell of its region can be solid (lbm_kernels.hpp tile_near_solid, called by
TileFrame with the ring of the kernel's first level); where the answer is no, the block skips the geometry lookup and interior tiles
take the LEAN path, which has no solid, ghost or validity logic at all. The mask query rounds outward to 8x8 blocks, aligned in a
strip to the first row of the strip's mask window (own rows +- GR, lbm_geom.hpp pack_mask), so a ring or a window a cell or two short
shows only at particular alignments of obstacle, tile origin and strip offset. The sweeps below visit every alignment: one solid cell
at EVERY position of a horizontal, a vertical and a diagonal line that cross several tile pitches of every kernel family
(whole domain), of three columns that cross both faces of a group of strips by +-16 rows and more (ghost zones and the rows just
outside a strip's window included), the smallest analytic discs (radius 0, 1, 2 cells: the disc branch of tile_near_solid) on the
same lines, and single cells in the corners, next to them and on the four boundaries.

References: the CPU oracle on the same mask (strict plans bit for bit, contracted ones within 1e-10); fp32 (tests/test_gpu_f32_oracle.py holds it to a float32 reference) is
held bit for bit to one k_step_site launch per iteration in the same arithmetic, as tests/test_gpu_random.py does.
A failing item reports every position that failed, so that the distance to the nearest tile origin / face names the short level.

The guard at the end runs without a GPU: the position lists are contiguous with the stated extents, and the oracle is stable at
every position (a reference that blew up would make `first_unstable_step() == -1` unreachable)."""
import collections
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

from oracle.oracle import Oracle, make_params
from tests.helpers import PKG, PLANS, TALL_F32, U_BAR_ABS, lbm_gpu, reference_problems, strict, u_bar_rel, where  # noqa: F401
from tests.reference import les_collide, oracle_run

gpu = pytest.mark.gpu          # (every test but the guard at the end of the module)

NX, NY = 224, 112              # >= three tiles in each direction for every shape (LEAN tiles exist); 224 % 64 != 0: a ragged last column
NY_TALL = 176                  # fp32 64x48 regions: an interior tall tile exists
STEPS, OF = 20, 16             # two deep launches and a remainder; force samples at t = 0 and 16
KW = dict(inlet_velocity=0.05)
KW_LES = dict(tau=0.51, inlet_velocity=0.08)
CS = 0.17
BOUNDS = [(0, 37), (37, 22), (59, 53)]      # faces at rows 37 and 59

LINES = {
    "horizontal": [(x, 50) for x in range(40, 150)],          # longer than a tile pitch + 2 x (ring 7 + block 8)
    "vertical": [(101, y) for y in range(8, 104)],
    "diagonal": [(40 + k, 20 + k) for k in range(70)],        # crosses the corners of regions
}
LINES_TALL = dict(LINES, vertical=[(101, y) for y in range(8, 168)])
FACE_COLUMNS = {x: [(x, y) for y in range(20, 80)] for x in (101, 0, 223)}     # -17 .. +20 rows around both faces
CORNERS = [(0, 0), (223, 0), (0, 111), (223, 111), (1, 1), (222, 110), (0, 50), (223, 50), (101, 0), (101, 111)]
INLET_CELLS = [p for p in CORNERS if p[0] == 0]
DISC_RADII = {0: 1, 1: 5, 2: 13}            # radius in cells -> solid cells of the disc

WHOLE_PLANS = ["rowil-site-nt", "planar-fuse3-8", "rowil-fuse4-nt-xcd", "rowil-deep6-nt", "planar-deep7-alt", "rowil-deep8-nt",
               "rowil-col5-nt", "planar-col6-alt", "rowil-col7-alt", "fast-rowil-col6", "fast-rowil-deep7", "fast-rowil-col7"]
FAMILY = {"site": "k_step_site<", "fuse3": "k_step3_tile<", "fuse4": "k_step4_tile<", "deep": "k_stepd_tile<", "col": "k_stepc_col<"}
LES_PLANS = ["rowil-col5-nt", "fast-rowil-col6"]
DISC_PLANS = ["rowil-col5-nt", "planar-col6-alt", "rowil-deep6-nt", "fast-rowil-col6"]
CORNER_PLANS = ["rowil-col5-nt", "rowil-deep6-nt"]
STRIP_CONFIGS = {
    "col5-halo0": ("rowil-col5-nt", dict(deep_halo=0, overlap=1)),
    "col5-halo1": ("rowil-col5-nt", dict(deep_halo=1, overlap=1)),
    "col5-halo2": ("rowil-col5-nt", dict(deep_halo=2, overlap=1)),
    "col5-halo2-serial": ("rowil-col5-nt", dict(deep_halo=2, overlap=0)),
    "col7": ("rowil-col5-nt", dict(deep=9, overlap=1)),
    "deep8": ("rowil-deep8-nt", dict(overlap=1)),
    "fuse3": ("rowil-fuse3-12-nt-xcd", dict(overlap=1)),
    "fast-col6-halo2": ("fast-rowil-col6", dict(deep_halo=2, overlap=1)),
    "fast-col6-halo2-serial": ("fast-rowil-col6", dict(deep_halo=2, overlap=0)),
}
SITE_F32 = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)

Ref = collections.namedtuple("Ref", "f_next rho ux uy forces bad count tmax solid")
Run = collections.namedtuple("Run", "count bad log f rho ux uy kernel solid")


def one_cell(x, y, ny=NY):
    m = np.zeros((ny, NX), np.uint8)
    m[y, x] = 1
    return m


def family(plan):
    o = PLANS[plan]
    deep = o.get("deep", 0)
    return "col" if deep >= 6 else "deep" if deep else {1: "site", 3: "fuse3", 4: "fuse4"}[o.get("fuse", 1)]


def disc_params(x, y, r):
    """cylinder_* fractions whose integer centre (lbmo_cylinder_x_cells / _y_cells) is (x, y) and whose radius is r cells."""
    return dict(cylinder_x=(x + 0.5) / NX, cylinder_y=(y + 0.5) / NY, cylinder_radius=(r + 0.5) / NY)


def parabolic():
    return importlib.import_module(PKG).parabolic_profile(NY, KW["inlet_velocity"])


@functools.lru_cache(maxsize=112)      # (the longest line has 110 positions; the items are ordered line by line, plans innermost)
def reference(kind, x, y, r=0):
    """The oracle with one solid cell at (x, y) — tests/reference.py oracle_run, "bgk": as it is; "les": with les_collide; "profile":
    with the parabolic inlet — or, "disc", the plain C oracle (Oracle.run) on the analytic disc of radius r cells centred there.
    Computed once per position, shared by every plan, read-only."""
    tmax, solid = None, None
    if kind != "disc":
        if kind == "bgk":
            run = oracle_run(NX, NY, STEPS, OF, mask=one_cell(x, y), **KW)
        elif kind == "les":
            run = oracle_run(NX, NY, STEPS, OF, mask=one_cell(x, y), collide=functools.partial(les_collide, cs=CS), **KW_LES)
        else:
            run = oracle_run(NX, NY, STEPS, OF, mask=one_cell(x, y), u=parabolic(), **KW)
        f, rho, ux, uy, forces = run.f_next, run.rho, run.ux, run.uy, run.forces
        bad, count, tmax = run.first_unstable, run.solid_count, run.tau_max
    else:
        p = make_params(NX, NY, **KW, **disc_params(x, y, r))
        o = Oracle(p)
        cells = tuple(getattr(o.L, "lbmo_cylinder_%s_cells" % k)(C.byref(p)) for k in ("x", "y", "radius"))
        assert cells == (x, y, r), (cells, x, y, r)
        rows = []
        bad = o.run(STEPS, OF, rows)
        f, rho, ux, uy, count, solid = o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy(), o.solid_count(), o.solid.copy()
        forces = [row[:3] for row in rows]
        o.close()
    for a in (f, rho, ux, uy):
        a.flags.writeable = False
    return Ref(f, rho, ux, uy, forces, bad, count, tmax, solid)


def run(lbm, opts, mask, nx=NX, ny=NY, bounds=None, **kw):
    """STEPS iterations, force samples every OF, of a whole-domain context or (bounds) an in-process group of strips."""
    make = lbm.Context(nx, ny, options=opts, solid=mask, **kw) if bounds is None else \
        lbm.Group(nx, ny, bounds, options=opts, solid=mask, **kw)
    with make as ctx:
        count = ctx.initialise()
        ctx.step(STEPS, OF)
        bad = ctx.first_unstable_step()
        log = ctx.drain_force_log()
        f = ctx.populations("f_next")
        rho, ux, uy = ctx.macros()
        kernel = ctx.kernel_name() if bounds is None else None
        solid = ctx.solid() if bounds is None else None
    return Run(count, bad, log, f, rho, ux, uy, kernel, solid)


def oracle_problems(got, ref, plan, les=False):
    """What of a run misses the oracle: stable; the solid count; then reference_problems of tests/helpers.py — forces, f_next, rho and
    u at the bars of test_masks_against_the_oracle (LES: of test_les_against_the_reference), contracted rho within 1e-10."""
    out = []
    if got.count != ref.count:
        out.append("solid count %d, reference %d" % (got.count, ref.count))
    if got.bad != -1 or ref.bad != -1:
        out.append("first unstable step %d, reference %d" % (got.bad, ref.bad))
    return out + reference_problems(plan, got.f, (got.rho, got.ux, got.uy), got.log, ref, U_BAR_ABS if les else u_bar_rel(ref))


def site_problems(got, ref):
    """fp32: what of a run differs from one k_step_site launch per iteration in the same arithmetic (bit for bit, forces included)."""
    out = []
    if got.count != 1 or ref.count != 1:
        out.append("solid counts %d / %d" % (got.count, ref.count))
    if got.bad != -1 or ref.bad != -1:
        out.append("first unstable step %d, site kernel %d" % (got.bad, ref.bad))
    if got.log != ref.log:
        out.append("force log %s, site kernel %s" % (got.log, ref.log))
    if not (np.all(np.isfinite(ref.f)) and np.array_equal(got.f, ref.f)):
        out.append("f_next is not the site kernel's bit for bit: " + where(got.f, ref.f))
    for a, b in ((got.rho, ref.rho), (got.ux, ref.ux), (got.uy, ref.uy)):
        if not np.array_equal(a, b):
            out.append("macros differ")
            break
    return out


def report(failures, total):
    assert not failures, "%d of %d positions failed:\n" % (len(failures), total) + "\n".join("  (%d, %d): %s" % f for f in failures)


# ---- 1. one solid cell swept across tile boundaries, whole domain -------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", WHOLE_PLANS)
@pytest.mark.parametrize("line", list(LINES))
def test_one_cell_swept_across_tiles(lbm, line, plan):
    failures = []
    for x, y in LINES[line]:
        mask = one_cell(x, y)
        got = run(lbm, PLANS[plan], mask, **KW)
        bad = oracle_problems(got, reference("bgk", x, y), plan)
        if not got.kernel.replace(" ", "").startswith(FAMILY[family(plan)]):
            bad.append("kernel " + got.kernel)
        if not np.array_equal(got.solid, mask):
            bad.append("solid() is not the mask")
        failures += [(x, y, b) for b in bad]
    report(failures, len(LINES[line]))


@gpu
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("line", list(LINES_TALL))
def test_one_cell_swept_across_tall_fp32_regions(lbm, line, arith):
    """fp32 on 64x48 regions (seven iterations per launch), strict and contracted, against the fp32 site kernel."""
    failures = []
    for x, y in LINES_TALL[line]:
        mask = one_cell(x, y, NY_TALL)
        ref = run(lbm, dict(SITE_F32, arith=arith), mask, ny=NY_TALL, precision="f32", **KW)
        got = run(lbm, dict(TALL_F32, arith=arith), mask, ny=NY_TALL, precision="f32", **KW)
        bad = site_problems(got, ref)
        if not (got.kernel.replace(" ", "").startswith("k_stepc_col<float,") and ref.kernel.startswith("k_step_site<float")):
            bad.append("kernels %s / %s" % (got.kernel, ref.kernel))
        failures += [(x, y, b) for b in bad]
    report(failures, len(LINES_TALL[line]))


@gpu
@pytest.mark.parametrize("plan", LES_PLANS)
def test_one_cell_swept_across_tiles_les(lbm, plan):
    """The Smagorinsky instantiations share the prologue: the horizontal line against the LES reference (tests/reference.py les_collide)."""
    failures = []
    for x, y in LINES["horizontal"]:
        ref = reference("les", x, y)
        got = run(lbm, PLANS[plan], one_cell(x, y), smagorinsky=CS, **KW_LES)
        bad = oracle_problems(got, ref, plan, les=True)
        if not got.kernel.endswith((",2>", ",3>")):
            bad.append("kernel " + got.kernel)
        if not ref.tmax > KW_LES["tau"]:       # the model is active
            bad.append("tau_eff never left tau")
        failures += [(x, y, b) for b in bad]
    report(failures, len(LINES["horizontal"]))


# ---- 2. the same cell swept across strip faces ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("config", list(STRIP_CONFIGS))
@pytest.mark.parametrize("column", list(FACE_COLUMNS))
def test_one_cell_swept_across_strip_faces(lbm, column, config):
    """Three uneven strips (faces at rows 37 and 59), each with its own mask window: the cell walks from 17 rows below the first face
    to 20 above the second, through both ghost zones — also where it lies ONLY in a neighbour's ghost zone, 7 to 12 rows from a
    face — on an interior column and on the inlet and outlet columns. Against the whole-domain oracle."""
    plan, extra = STRIP_CONFIGS[config]
    failures = []
    for x, y in FACE_COLUMNS[column]:
        got = run(lbm, dict(PLANS[plan], **extra), one_cell(x, y), bounds=BOUNDS, **KW)
        failures += [(x, y, b) for b in oracle_problems(got, reference("bgk", x, y), plan)]
    report(failures, len(FACE_COLUMNS[column]))


# ---- 3. the smallest analytic discs ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", DISC_PLANS)
@pytest.mark.parametrize("r", list(DISC_RADII))
@pytest.mark.parametrize("line", ["horizontal", "vertical"])
def test_smallest_discs_swept_across_tiles(lbm, line, r, plan):
    """No mask: the disc branch of tile_near_solid (exact, not block-rounded) with discs smaller than a ring — radius 0, 1 and 2
    cells, i.e. 1, 5 and 13 solid cells — centred on every position of the lines of part 1. Against the plain C oracle."""
    failures = []
    for x, y in LINES[line]:
        ref = reference("disc", x, y, r)
        got = run(lbm, PLANS[plan], None, **KW, **disc_params(x, y, r))
        bad = oracle_problems(got, ref, plan)
        if ref.count != DISC_RADII[r]:
            bad.append("the oracle's disc has %d cells" % ref.count)
        if not np.array_equal(got.solid, ref.solid):
            bad.append("solid() is not the oracle's disc")
        failures += [(x, y, b) for b in bad]
    report(failures, len(LINES[line]))


# ---- 4. corners and walls --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("plan", CORNER_PLANS)
def test_one_cell_in_corners_and_on_walls(lbm, plan):
    """Single cells in the four corners, one cell inside two of them and on the inlet, the outlet and both walls: the LEAN bounds
    X0 >= HW + 1, yg0 >= HW + 1 and their upper twins. The inlet-column cells also under a parabolic inlet profile."""
    failures = []
    for x, y in CORNERS:
        got = run(lbm, PLANS[plan], one_cell(x, y), **KW)
        failures += [(x, y, b) for b in oracle_problems(got, reference("bgk", x, y), plan)]
    for x, y in INLET_CELLS:
        got = run(lbm, PLANS[plan], one_cell(x, y), inlet_profile=parabolic(), **KW)
        failures += [(x, y, "parabolic inlet: " + b) for b in oracle_problems(got, reference("profile", x, y), plan)]
    report(failures, len(CORNERS) + len(INLET_CELLS))


@gpu
@pytest.mark.parametrize("arith", [0, 1])
def test_one_cell_in_corners_and_on_walls_fp32(lbm, arith):
    failures = []
    for x, y, u in [(x, y, None) for x, y in CORNERS] + [(x, y, parabolic()) for x, y in INLET_CELLS]:
        kw = dict(KW, precision="f32", inlet_profile=u)
        ref = run(lbm, dict(SITE_F32, arith=arith), one_cell(x, y), **kw)
        got = run(lbm, dict(TALL_F32, arith=arith), one_cell(x, y), **kw)
        failures += [(x, y, ("parabolic inlet: " if u is not None else "") + b) for b in site_problems(got, ref)]
    report(failures, len(CORNERS) + len(INLET_CELLS))


# ---- 5. the guard: no GPU ----------------------------------------------------------------------------------------------------------
def test_position_lists_are_contiguous():
    h, v, d = LINES["horizontal"], LINES["vertical"], LINES["diagonal"]
    assert h == [(x, 50) for x in range(40, 150)] and len(h) == 110
    assert v == [(101, y) for y in range(8, 104)] and len(v) == 96
    assert d == [(40 + k, 20 + k) for k in range(70)] and d[0] == (40, 20) and d[-1] == (109, 89)
    assert LINES_TALL["horizontal"] == h and LINES_TALL["diagonal"] == d
    assert LINES_TALL["vertical"] == [(101, y) for y in range(8, 168)] and len(LINES_TALL["vertical"]) == 160
    for line in list(LINES.values()) + list(LINES_TALL.values()) + list(FACE_COLUMNS.values()):
        steps = {(b[0] - a[0], b[1] - a[1]) for a, b in zip(line, line[1:])}
        assert len(steps) == 1 and steps <= {(1, 0), (0, 1), (1, 1)}, steps          # contiguous: no position skipped
        assert len(set(line)) == len(line)
    # a line is longer than the widest tile pitch (64) plus twice (ring 7 + block 8) / than three of the tallest fp64 regions' pitch
    assert len(h) > 64 + 2 * (7 + 8) and len(v) > 3 * 22 and NX % 64 != 0 and NX >= 3 * 64 and NY >= 3 * 32 and NY_TALL >= 3 * 48
    assert sorted(FACE_COLUMNS) == [0, 101, 223] and FACE_COLUMNS[223][0] == (223, 20) and FACE_COLUMNS[223][-1] == (223, 79)
    faces = [y0 for y0, _ in BOUNDS[1:]]
    assert faces == [37, 59] and sum(n for _, n in BOUNDS) == NY and [y0 for y0, _ in BOUNDS] == [0, 37, 59]
    for x, col in FACE_COLUMNS.items():
        rows = [y for _, y in col]
        assert all(c[0] == x for c in col) and rows == list(range(20, 80))
        for face in faces:                       # every distance from -16 to +16 rows around both faces
            assert set(range(-16, 17)) <= {y - face for y in rows}
    assert set(FACE_COLUMNS[101]) <= set(LINES["vertical"])      # (the references of part 1 again)
    assert len(CORNERS) == len(set(CORNERS)) == 10 and INLET_CELLS == [(0, 0), (0, 111), (0, 50)]
    assert all(0 <= x < NX and 0 <= y < NY for x, y in CORNERS)
    assert {strict(p) for p in WHOLE_PLANS} == {True, False} and {family(p) for p in WHOLE_PLANS} == set(FAMILY)
    assert all(p in PLANS for p in WHOLE_PLANS + LES_PLANS + DISC_PLANS + CORNER_PLANS + [c[0] for c in STRIP_CONFIGS.values()])


@pytest.mark.parametrize("name", list(LINES) + ["column-0", "column-223", "corners"])
def test_the_oracle_is_stable_at_every_position(name):
    cells = LINES[name] if name in LINES else CORNERS if name == "corners" else FACE_COLUMNS[int(name.split("-")[1])]
    for x, y in cells:
        ref = reference("bgk", x, y)
        assert ref.bad == -1 and ref.count == 1 and [r[0] for r in ref.forces] == [0, 16], (x, y)
        assert np.all(np.isfinite(ref.f_next))
    if name == "corners":
        for x, y in INLET_CELLS:
            assert reference("profile", x, y).bad == -1, (x, y)


# (the LES reference is numpy, a quarter of a second per position: its stability and tau_eff > tau are asserted position by position
# where it is used, in test_one_cell_swept_across_tiles_les)


@pytest.mark.parametrize("r", list(DISC_RADII))
@pytest.mark.parametrize("line", ["horizontal", "vertical"])
def test_the_smallest_discs_are_what_they_are_meant_to_be(line, r):
    for x, y in LINES[line]:
        ref = reference("disc", x, y, r)      # (asserts the oracle's integer centre and radius)
        assert ref.count == DISC_RADII[r] == int(ref.solid.sum()) and ref.bad == -1 and ref.solid[y, x] == 1, (x, y, r)
