"""Point probes on the GPU (lbm_probes_begin / k_probes): (rho, ux, uy) interpolated bilinearly at chosen points into a device ring at
the force-output iterations of step(n, of), against `macros()` of a SECOND context stepped to t + 1 and interpolated by numpy in float64
with the formula of include/lbm_hip.h:

    x0 = floor(px), fx = px - x0, x1 = min(x0 + 1, nx - 1);   y likewise with ny - 1
    a = (1 - fx) v(x0, y0) + fx v(x1, y0);   b = (1 - fx) v(x0, y1) + fx v(x1, y1);   v = (1 - fy) a + fy b

every product and sum rounded to double, a term of weight zero left out. Every comparison is np.array_equal: there is no tolerance.
The twin runs the probed context's arithmetic (and, in fp32, its plan: fp32 has no oracle that ties its plans together bit for bit;
the fp64 plans of one arithmetic mode compute the same populations to the bit, tests/test_gpu_parity.py). Grids are 128x32 and 256x64
with the default disc, the sizes of goldens g1 and g2."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import EXE, PKG, PLANS

pytestmark = pytest.mark.gpu

GRIDS = [(128, 32), (256, 64)]
STEPS, OF = 23, 5
POINTS_T = [0, 5, 10, 15, 20]
PROBES_MAX = 65536


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    assert pkg.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert hasattr(pkg.Context, "probes_begin")
    return pkg


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def interpolate(macros, xy):
    """[n, 3] float64: the definition, elementwise in numpy (every product and every sum is one IEEE double operation)."""
    xy = np.asarray(xy, dtype=np.float64)
    ny, nx = macros[0].shape
    x0, y0 = np.floor(xy[:, 0]).astype(np.int64), np.floor(xy[:, 1]).astype(np.int64)
    fx, fy = xy[:, 0] - x0, xy[:, 1] - y0
    x1, y1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1)
    out = np.empty((len(xy), 3), dtype=np.float64)
    for k, v in enumerate(macros):
        v = np.asarray(v, dtype=np.float64)
        a = np.where(fx == 0.0, v[y0, x0], (1.0 - fx) * v[y0, x0] + fx * v[y0, x1])
        b = np.where(fx == 0.0, v[y1, x0], (1.0 - fx) * v[y1, x0] + fx * v[y1, x1])
        out[:, k] = np.where(fy == 0.0, a, (1.0 - fy) * a + fy * b)
    return out


def interpolate_loop(macros, xy):
    """The same, probe by probe with scalar float64 arithmetic and the zero-weight terms really left out (a check of `interpolate`)."""
    ny, nx = macros[0].shape
    out = np.empty((len(xy), 3), dtype=np.float64)
    for j, (px, py) in enumerate(np.asarray(xy, dtype=np.float64)):
        x0, y0 = int(np.floor(px)), int(np.floor(py))
        fx, fy = np.float64(px - x0), np.float64(py - y0)
        x1, y1 = min(x0 + 1, nx - 1), min(y0 + 1, ny - 1)
        for k, v in enumerate(macros):
            a = v[y0, x0] if fx == 0.0 else (1.0 - fx) * v[y0, x0] + fx * v[y0, x1]
            if fy != 0.0:
                b = v[y1, x0] if fx == 0.0 else (1.0 - fx) * v[y1, x0] + fx * v[y1, x1]
                a = (1.0 - fy) * a + fy * b
            out[j, k] = a
    return out


_twins = {}


def twin_macros(lbm, nx, ny, precision, options):
    """{t: macros() of a second context stepped to t + 1}: one run per grid, precision and options, shared and left unchanged."""
    key = (nx, ny, precision, tuple(sorted((options or {}).items())))
    if key not in _twins:
        out = {}
        with lbm.Context(nx, ny, precision=precision, options=options) as tw:
            tw.initialise()
            for t in POINTS_T:
                tw.step(t + 1 - tw.steps_done)
                out[t] = tw.macros()
        _twins[key] = out
    return _twins[key]


_solid = {}


def solid_of(lbm, nx, ny):
    if (nx, ny) not in _solid:
        with lbm.Context(nx, ny, options=dict(tune=0)) as c:
            c.initialise()
            _solid[(nx, ny)] = np.asarray(c.solid()).reshape(ny, nx).astype(bool)
    return _solid[(nx, ny)]


def probe_points(lbm, nx, ny):
    """The table of the issue; the names say what each point covers."""
    s = solid_of(lbm, nx, ny)
    cx, cy = int(0.2 * nx), int(0.5 * ny)
    assert s[cy, cx]
    one = [(x, y) for y in range(ny - 1) for x in range(nx - 1) if int(s[y, x]) + int(s[y, x + 1]) + int(s[y + 1, x]) + int(s[y + 1, x + 1]) == 1]
    assert one, "the disc has a cell square with exactly one solid corner"
    named = {
        "interior node": (nx // 2 + 7.0, ny // 2 - 5.0),
        "inlet node": (0.0, 5.0), "outlet node": (nx - 1.0, 5.0),
        "bottom wall": (33.0, 0.0), "top wall": (33.0, ny - 1.0), "bottom wall between nodes": (33.5, 0.0), "top wall between nodes": (34.25, ny - 1.0),
        "corner": (nx - 1.0, ny - 1.0), "origin": (0.0, 0.0), "inlet top corner": (0.0, ny - 1.0), "outlet bottom corner": (nx - 1.0, 0.0),
        "node in the disc": (float(cx), float(cy)),
        "one solid corner": (one[0][0] + 0.375, one[0][1] + 0.625),
        "tile edge in x": (63.5, 15.5),
        "inlet and wall corner": (0.5, 0.5), "outlet and wall corner": (nx - 1.5, ny - 1.5),
        "inlet between rows": (0.0, 9.25), "outlet between rows": (nx - 1.0, 9.5), "next to the outlet": (nx - 1.25, 20.0),
        # strips of 16 + 16 / 10 + 22 rows: y1 on the north ghost row, on the outlet column the row beyond it; nodes on the face rows
        "across the 16+16 face": (5.0, 15.5), "across the face on the outlet": (nx - 1.0, 15.5), "across the face on the inlet": (0.0, 15.75),
        "across the face, four cells": (70.5, 15.25), "node on the face row": (40.0, 15.0), "node above the face": (41.0, 16.0),
        "node on the 10+22 face row": (40.0, 9.0), "across the 10+22 face": (44.125, 9.875),
    }
    rake = [(100.25, y) for y in np.linspace(0.0, ny - 1.0, 64)]      # several points per column of cells
    return list(named), np.array(list(named.values()) + rake, dtype=np.float64)


def run_probes(ctx, xy, calls=((STEPS, OF),), capacity=8):
    ctx.initialise()
    ctx.probes_begin(xy, capacity)
    for n, of in calls:
        ctx.step(n, of)
    return ctx.drain_probes()


def test_the_vectorised_reference_is_the_scalar_loop(lbm):
    nx, ny = GRIDS[0]
    _, xy = probe_points(lbm, nx, ny)
    m = twin_macros(lbm, nx, ny, "f64", dict(tune=0, arith=0))[20]
    assert np.array_equal(interpolate(m, xy), interpolate_loop(m, xy))
    assert np.max(np.abs(m[2])) > 1e-6      # a flow with uy = 0 would hide a swapped weight


# ---- 5. every sample of every probe -------------------------------------------------------------------------------------------------
MODES = {"fp64-strict": ("f64", 0), "fp64-contracted": ("f64", 1), "fp32": ("f32", 1)}
PINNED = {"measured": None,
          "deep=6": dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=6),
          "deep=1": dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=1),
          "fuse=3": dict(tune=0, layout=1, nt=1, alternate=0, fuse=3, pair_ty=12, xcd=1),
          "single": dict(tune=0, layout=1, nt=1, alternate=0, fuse=1)}


@pytest.mark.parametrize("plan", list(PINNED))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_every_sample_of_every_probe_equals_the_interpolated_twin(lbm, grid, mode, plan):
    nx, ny = grid
    precision, arith = MODES[mode]
    names, xy = probe_points(lbm, nx, ny)
    opts = dict(PINNED[plan] or {}, arith=arith)
    with lbm.Context(nx, ny, precision=precision, options=opts) as c:
        ts, vals = run_probes(c, xy)
        assert c.first_unstable_step() == -1 and c.probes_count() == len(xy) and c.probes_pending() == 0
        if plan == "measured":      # the twin of a measured plan runs that very plan
            opts = dict(c.plan_options(), tune=0, arith=arith)
    assert ts.tolist() == POINTS_T and vals.shape == (5, len(xy), 3) and vals.dtype == np.float64
    # fp64: every plan of one arithmetic mode computes the same populations, so one twin per mode serves them all
    tw = twin_macros(lbm, nx, ny, precision, opts if precision == "f32" else dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=arith))
    s = solid_of(lbm, nx, ny)
    for k, t in enumerate(POINTS_T):
        ref = interpolate(tw[t], xy)
        bad = np.argwhere(vals[k] != ref)
        assert np.array_equal(vals[k], ref), (t, [(names[j] if j < len(names) else f"rake {j - len(names)}", xy[j].tolist(), vals[k][j, q], ref[j, q]) for j, q in bad[:6]])
        j = names.index("node in the disc")
        assert vals[k][j].tolist() == [1.0, 0.0, 0.0]
        j = names.index("interior node")      # a node returns its cell's macros bit for bit
        x, y = int(xy[j][0]), int(xy[j][1])
        assert not s[y, x] and vals[k][j].tolist() == [tw[t][0][y, x], tw[t][1][y, x], tw[t][2][y, x]]
    assert np.any(vals[-1][:, 2] != 0.0) and not np.array_equal(vals[0], vals[-1])      # a flow at rest would hide a swapped weight


# ---- 6. strips ----------------------------------------------------------------------------------------------------------------------
STRIP_PLANS = ["rowil-site-nt", "rowil-fuse3-12-nt-xcd"]
_whole = {}


def whole_samples(lbm, nx, ny):
    if (nx, ny) not in _whole:
        _, xy = probe_points(lbm, nx, ny)
        with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"]) as c:
            _whole[(nx, ny)] = run_probes(c, xy)
    return _whole[(nx, ny)]


@pytest.mark.parametrize("plan", STRIP_PLANS)
def test_a_group_of_two_strips_adds_up_to_the_whole_domain(lbm, plan):
    """16 + 16 rows on one device, peer transport (the one a group has on a single GPU): every probe is sampled by the strip that owns
    floor(py) and reported as +0.0 by the other; the probes across the face read the owner's north ghost row, the one on the outlet column
    the row beyond it, and the node on the face row reads no ghost row."""
    nx, ny = GRIDS[0]
    names, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    with lbm.Group(nx, ny, [(0, 16), (16, 16)], options=PLANS[plan]) as g:
        g.initialise()
        g.probes_begin(xy, 8)
        g.step(STEPS, OF)
        assert g.first_unstable_step() == -1 and g.probes_pending() == 5 and g.probes_count() == len(xy)
        parts = [c.drain_probes() for c in g.ctxs]
        assert g.probes_pending() == 0
    lower = np.floor(xy[:, 1]) < 16
    for (t, v), mine in zip(parts, (lower, ~lower)):
        assert t.tolist() == wt.tolist() == POINTS_T
        assert np.array_equal(v[:, mine], wv[:, mine])                                  # the owner alone holds the whole domain's sample
        assert not v[:, ~mine].any() and not np.signbit(v[:, ~mine]).any()              # +0.0 from the other strip
    assert np.array_equal(parts[0][1] + parts[1][1], wv)
    for name in ("across the 16+16 face", "across the face on the outlet", "across the face on the inlet", "node on the face row"):
        assert lower[names.index(name)]


def test_group_drain_sums_its_members(lbm):
    nx, ny = GRIDS[0]
    _, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    with lbm.Group(nx, ny, [(0, 16), (16, 16)], options=PLANS["rowil-site-nt"], probes=xy, probe_capacity=8) as g:      # the keyword: begun by initialise()
        g.initialise()
        g.step(STEPS, OF)
        first = g.drain_probes(2)
        rest = g.drain_probes()
    assert first[0].tolist() == [0, 5] and rest[0].tolist() == [10, 15, 20]
    assert np.array_equal(np.concatenate([first[1], rest[1]]), wv)


def test_host_staged_strips_of_10_and_22_rows_add_up_to_the_whole_domain(lbm):
    """10 + 22 rows. A group refuses a strip of fewer than twelve rows (two exchanges' worth), so this decomposition runs as the
    MPI-hosted calling pattern: two contexts, one iteration per call, lbm_halo_export / lbm_halo_import between the calls."""
    nx, ny = GRIDS[0]
    names, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    bounds = [(0, 10), (10, 22)]
    with pytest.raises(lbm.LbmError, match="needs at least 12 rows"):
        lbm.Group(nx, ny, bounds, options=PLANS["rowil-site-nt"])
    ctxs = [lbm.Context(nx, ny, y_start=y0, local_ny=n, options=PLANS["rowil-site-nt"]) for y0, n in bounds]
    try:
        for c in ctxs:
            c.initialise()
            c.probes_begin(xy, 8)

        def exchange():
            ex = [c.halo_export(south=(k > 0), north=(k < 1)) for k, c in enumerate(ctxs)]
            ctxs[0].halo_import(south=None, north=ex[1][0])
            ctxs[1].halo_import(south=ex[0][1], north=None)
        exchange()
        for _ in range(STEPS):
            for c in ctxs:
                c.step(1, OF)
            exchange()
        parts = [c.drain_probes() for c in ctxs]
    finally:
        for c in ctxs:
            c.close()
    lower = np.floor(xy[:, 1]) < 10
    for (t, v), mine in zip(parts, (lower, ~lower)):
        assert t.tolist() == POINTS_T
        assert np.array_equal(v[:, mine], wv[:, mine]) and not v[:, ~mine].any()
    assert np.array_equal(parts[0][1] + parts[1][1], wv)
    assert lower[names.index("across the 10+22 face")] and lower[names.index("node on the 10+22 face row")] and lower[names.index("outlet between rows")]


@pytest.mark.parametrize("overlap", [1, 0])
def test_the_rccl_loopback_context_gives_the_whole_domains_samples(lbm, overlap):
    """The RCCL transport on one GPU: a one-rank communicator sending its edge rows to itself (loopback=2). The sample is queued behind
    the exchange's join like the force kernel; the walls' conditions hide the looped-back ghost rows, so the flow is the whole domain's."""
    nx, ny = GRIDS[0]
    _, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    with lbm.Context(nx, ny, options=dict(PLANS["rowil-fuse3-12-nt-xcd"], loopback=2, overlap=overlap)) as c:
        c.comm_init(0, 1, c.comm_unique_id())
        t, v = run_probes(c, xy)
        assert c.first_unstable_step() == -1
    assert t.tolist() == wt.tolist() and np.array_equal(v, wv)


# ---- 7. the ring --------------------------------------------------------------------------------------------------------------------
def test_the_ring_fills_drains_oldest_first_and_resets(lbm):
    nx, ny = GRIDS[0]
    _, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"]) as c:
        c.initialise()
        assert c.probes_count() == 0 and c.probes_pending() == 0 and c.drain_probes()[1].shape == (0, 0, 3)      # never begun
        c.probes_begin(xy, capacity=2)
        c.step(10, 5)                                                      # t = 0, 5 fill the ring; t = 10 finds it full
        assert c.probes_pending() == 2
        with pytest.raises(lbm.LbmError, match=r"lbm_hip error -1: probe ring full \(2 samples\): drain it \(lbm_drain_probes\)"):
            c.step(1, 5)
        assert c.steps_done == 10 and c.probes_pending() == 2
        t, v = c.drain_probes(1)                                           # the oldest sample; one stays
        assert t.tolist() == [0] and np.array_equal(v[0], wv[0]) and c.probes_pending() == 1
        c.step(1, 5)                                                       # t = 10 goes into the slot that was freed (the ring wraps)
        t, v = c.drain_probes()
        assert t.tolist() == [5, 10] and np.array_equal(v, wv[1:3]) and c.probes_pending() == 0
        c.step(5, 5)                                                       # t = 15
        c.probes_end()
        c.step(5, 5)                                                       # t = 20: not sampled; the undrained sample stays
        assert c.probes_pending() == 1 and c.probes_count() == len(xy)
        t, v = c.drain_probes()
        assert t.tolist() == [15] and np.array_equal(v[0], wv[3])
        c.probes_begin(xy[:3], capacity=2)
        c.step(5, 5)                                                       # t = 25
        assert c.probes_pending() == 1
        c.probes_begin(xy[:7], capacity=2)                                 # again: new points, and the ring is empty
        assert c.probes_pending() == 0 and c.probes_count() == 7 and len(c.drain_probes()[0]) == 0
        c.step(5, 5)                                                       # t = 30
        t, v = c.drain_probes()
        assert t.tolist() == [30] and v.shape == (1, 7, 3)


def test_the_probes_keyword_and_bad_arguments(lbm):
    nx, ny = GRIDS[0]
    _, xy = probe_points(lbm, nx, ny)
    wt, wv = whole_samples(lbm, nx, ny)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], probes=xy[:5], probe_capacity=3) as c:
        c.initialise()
        c.step(6, 5)
        t, v = c.drain_probes()
        assert t.tolist() == [0, 5] and np.array_equal(v, wv[:2, :5])
        L, err = lbm.lib(), lambda: lbm.lib().lbm_last_error().decode()
        q = np.array([[1.0, 2.0], [128.0, 3.0]])
        for pts, n, cap, text in [(q, 2, 2, "probe 1: x = 128 outside the domain 0..127"), (q, 1, 0, "capacity 0 < 1"), (q, 0, 2, "n = 0 < 1"),
                                  (np.array([[1.0, np.nan]]), 1, 2, "probe 0: (1, nan) is not finite"), (np.array([[1.0, 31.5]]), 1, 2, "y = 31.5 outside the domain 0..31")]:
            assert L.lbm_probes_begin(c.h, lbm.binding._dp(pts), n, cap) == -1 and text in err(), (text, err())
        assert L.lbm_probes_begin(c.h, None, 1, 2) == -1 and "null" in err()
        big = np.zeros((PROBES_MAX + 1, 2))
        assert L.lbm_probes_begin(c.h, lbm.binding._dp(big), PROBES_MAX + 1, 2) == -1 and "n = 65537 > LBM_PROBES_MAX" in err()
        assert c.probes_count() == 5      # a refused call leaves the probes as they were
    with lbm.Context(nx, ny) as c:
        with pytest.raises(lbm.LbmError, match="initialised context"):
            c.probes_begin(xy)


# ---- 8. probes change reporting only ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-deep6-nt", "fast-rowil-col6"])
def test_probes_change_reporting_only(lbm, plan):
    nx, ny = GRIDS[1]
    _, xy = probe_points(lbm, nx, ny)

    def run(probes):
        with lbm.Context(nx, ny, options=PLANS[plan], probes=probes, probe_capacity=8) as c:
            c.initialise()
            c.stats_begin(0)
            c.frames_begin(4)
            c.step(STEPS, OF)
            return (c.populations("f_next"), c.macros(), c.drain_force_log(), c.stats_sums(), c.stats_samples(), c.drain_frames(), c.kernel_name(),
                    c.plan_options() if plan != "auto" else None)
    a, b = run(None), run(xy)
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2] == b[2] and len(a[2]) == 5
    assert np.array_equal(a[3], b[3]) and a[4] == b[4] == 5
    assert len(a[5]) == len(b[5]) == 5 and all(t == u and np.array_equal(f, g) for (t, f), (u, g) in zip(a[5], b[5]))
    assert a[6] == b[6] and a[7] == b[7]


# ---- 9. the largest n ---------------------------------------------------------------------------------------------------------------
def test_the_largest_number_of_probes(lbm):
    """n = LBM_PROBES_MAX random points on 256x64 (fixed seed; none kept away from the disc, the walls or the inlet and outlet), one sample."""
    nx, ny = GRIDS[1]
    rng = np.random.default_rng(20261018)
    xy = np.stack([rng.uniform(0.0, nx - 1.0, PROBES_MAX), rng.uniform(0.0, ny - 1.0, PROBES_MAX)], axis=1)
    xy[:64] = np.floor(xy[:64])                                  # some nodes,
    xy[64:96, 0] = np.floor(xy[64:96, 0])                        # some points on a column of nodes and some on a row,
    xy[96:128, 1] = np.floor(xy[96:128, 1])
    xy[128:160, 0], xy[160:192, 0] = 0.0, nx - 1.0               # the inlet and the outlet,
    xy[192:224, 1], xy[224:256, 1] = 0.0, ny - 1.0               # and the walls
    s = solid_of(lbm, nx, ny)
    x0, y0 = np.floor(xy[:, 0]).astype(int), np.floor(xy[:, 1]).astype(int)
    near = s[y0, x0] | s[y0, np.minimum(x0 + 1, nx - 1)] | s[np.minimum(y0 + 1, ny - 1), x0] | s[np.minimum(y0 + 1, ny - 1), np.minimum(x0 + 1, nx - 1)]
    assert near.sum() > 20, near.sum()                           # probes with solid corners are among them
    opts = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=0)
    with lbm.Context(nx, ny, options=opts) as c:
        c.initialise()
        c.step(20, 0)
        c.probes_begin(xy, 1)
        c.step(1, 5)                                             # t = 20
        t, v = c.drain_probes()
    assert t.tolist() == [20] and v.shape == (1, PROBES_MAX, 3)
    ref = interpolate(twin_macros(lbm, nx, ny, "f64", opts)[20], xy)
    assert np.array_equal(v[0], ref), np.argwhere(v[0] != ref)[:8]


# ---- 10. lbm_solver --probe-line ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--strips", "2"]], ids=["whole", "two-strips"])
def test_lbm_solver_writes_the_bindings_samples(lbm, tmp_path, extra):
    cmd = [EXE, "--nx", "128", "--ny", "32", "--steps", "21", "--output-frequency", "10", "--probe-line", "40", "2", "40", "29", "10", "--no-vtk"]
    r = subprocess.run(cmd + ["--no-tune", "--quiet"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    rows = open(tmp_path / "probes.csv").read().splitlines()
    assert rows[0] == "timestep,probe,x,y,rho,ux,uy" and len(rows) == 1 + 3 * 10
    got = np.array([[float(v) for v in ln.split(",")] for ln in rows[1:]])
    xy = np.array([(40.0, 2.0 + 3.0 * j) for j in range(10)])
    with lbm.Context(128, 32, options=dict(tune=0)) as c:      # the solver's defaults (LBM::SimulationParams) are the binding's
        c.initialise()
        c.probes_begin(xy, 4)
        c.step(21, 10)
        t, v = c.drain_probes()
    assert t.tolist() == [0, 10, 20]
    assert got[:, 0].tolist() == [float(u) for u in t for _ in range(10)] and got[:, 1].tolist() == [float(j) for _ in t for j in range(10)]
    assert np.array_equal(got[:, 2:4], np.tile(xy, (3, 1)))
    assert np.array_equal(got[:, 4:], v.reshape(30, 3))                # "%.17g" reads back to the very doubles
    assert not np.array_equal(v[2], v[0])
    assert not os.path.exists(tmp_path / "vtk_output")
