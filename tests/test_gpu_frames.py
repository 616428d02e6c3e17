"""Coarsened flow frames on the GPU (lbm_frames_begin / k_frame): rho, ux, uy and the vorticity d uy/dx - d ux/dy, block-averaged
k x k into a device ring at the force-output iterations of step(n, of), against a numpy operator applied to a TWIN context's macros().

The fine fields of the frame of iteration t are defined as the (rho, ux, uy) `macros()` returns on a context with steps_done == t + 1.
`reference_frame` below forms the vorticity (central differences inside, one-sided on the four edges of the domain) and the k x k
block means in float64. The bar is derived, not measured: any fixed summation order of k * k <= 4096 doubles differs from numpy's by a
few 1e-16 relative, so after the single rounding to float32 a plane differs from float32(ref) by at most one float ulp of its largest
value; the tests allow two: max|got - float32(ref)| <= 2.4e-7 * max|ref| per plane. Where two runs have bit-equal macros (plans within
one arithmetic mode, strips against the whole domain) their frames are compared with np.array_equal."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import EXE, PKG, PLANS, square

pytestmark = pytest.mark.gpu

BAR = 2.4e-7          # two float32 ulps (2 * 2^-23), relative to the plane's largest value
NX, NY = 192, 64
KW = dict(tau=0.6, inlet_velocity=0.05)
STEPS, OF = 90, 30
POINTS = [0, 30, 60]
PLANES = ("rho", "ux", "uy", "vorticity")


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    assert pkg.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert hasattr(pkg.Context, "frames_begin")
    return pkg


def vorticity(ux, uy):
    """d uy/dx - d ux/dy in float64: 0.5 * (v[+1] - v[-1]) inside, v[1] - v[0] and v[n-1] - v[n-2] on the edges of the domain."""
    def ddx(v):
        d = np.empty_like(v)
        d[:, 1:-1] = 0.5 * (v[:, 2:] - v[:, :-2])
        d[:, 0] = v[:, 1] - v[:, 0]
        d[:, -1] = v[:, -1] - v[:, -2]
        return d
    return ddx(uy) - ddx(ux.T).T


def reference_frame(macros, k):
    """The operator of the definition: [4, ny / k, nx / k] float64 block means of rho, ux, uy and the vorticity."""
    rho, ux, uy = (np.asarray(a, dtype=np.float64) for a in macros)
    ny, nx = rho.shape
    fine = np.stack([rho, ux, uy, vorticity(ux, uy)])
    return fine.reshape(4, ny // k, k, nx // k, k).sum(axis=(2, 4)) / float(k * k)


def check(got, ref, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    for j, name in enumerate(PLANES):
        err = float(np.max(np.abs(got[j].astype(np.float64) - ref[j].astype(np.float32).astype(np.float64))))
        bar = BAR * float(np.max(np.abs(ref[j])))
        print(f"{what} {name}: max err {err:.3e}, bar {bar:.3e}, max|ref| {np.max(np.abs(ref[j])):.3e}")
        assert err <= bar, (what, name, err, bar)


def twin_macros(make, points):
    """{t: macros() of a fresh context stepped to t + 1}"""
    out = {}
    with make() as tw:
        tw.initialise()
        for t in points:
            tw.step(t + 1 - tw.steps_done)
            out[t] = tw.macros()
    return out


def run_frames(make, k, calls=((STEPS, OF),), capacity=8):
    with make() as c:
        c.initialise()
        c.frames_begin(k, capacity)
        for n, of in calls:
            c.step(n, of)
        return c.drain_frames()


GEOMETRIES = {"disc": None, "square": square(NX, NY)}
_twins = {}


F32_PLAN = PLANS["rowil-deep6-nt"]      # fp32 has no oracle that ties its plans together bit for bit: the twin runs the frames' plan


def twins(lbm, geometry, precision="f64"):
    key = (geometry, precision)
    if key not in _twins:      # one reference run per geometry and precision, shared and left unchanged
        opts = F32_PLAN if precision == "f32" else None
        _twins[key] = twin_macros(lambda: lbm.Context(NX, NY, solid=GEOMETRIES[geometry], precision=precision, options=opts, **KW), POINTS)
    return _twins[key]


# ---- 1. against the reference operator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_frames_equal_the_operator_on_the_twins_macros(lbm, geometry, k):
    frames = run_frames(lambda: lbm.Context(NX, NY, solid=GEOMETRIES[geometry], **KW), k)
    assert [t for t, _ in frames] == POINTS
    tw = twins(lbm, geometry)
    for t, f in frames:
        ref = reference_frame(tw[t], k)
        check(f, ref, f"{geometry} k={k} t={t}")
        if t > 0:
            assert np.max(np.abs(f[3])) > 1e-4      # a frame with w = 0 cannot pass


def test_block_columns_and_row_bands_beyond_one_block(lbm):
    """nx = 520 is three blocks of columns at k = 2 (254 columns each) and five at k = 40 (80 each); 120 rows are several bands; at
    k = 40 a band is one row of coarse cells. Every block edge and band edge lies inside the flow."""
    nx, ny = 520, 120
    make = lambda: lbm.Context(nx, ny, inlet_velocity=0.06, cylinder_radius=0.12)
    tw = twin_macros(make, [0, 40])
    for k in (1, 2, 8, 40):
        frames = run_frames(make, k, calls=((60, 40),))
        assert [t for t, _ in frames] == [0, 40]
        for t, f in frames:
            check(f, reference_frame(tw[t], k), f"{nx}x{ny} k={k} t={t}")


# ---- 2. invariance ------------------------------------------------------------------------------------------------------------------
STRICT_PLANS = ["rowil-site-nt", "planar-fuse3-8", "rowil-deep6-nt", "rowil-col5-nt", "planar-col6-alt"]
FAST_PLANS = ["fast-site", "fast-rowil-fuse3-12-xcd", "fast-rowil-deep7", "fast-rowil-col6", "fast-planar-col5"]


@pytest.mark.parametrize("plans", [STRICT_PLANS, FAST_PLANS], ids=["strict", "contracted"])
def test_frames_do_not_depend_on_the_plan(lbm, plans):
    """One site, one fused-tile, one LDS-deep and both register-kernel plans per arithmetic mode. Within a mode every plan computes
    the same populations to the bit (tests/test_gpu_parity.py, tests/test_gpu_geometry.py), hence the same macros and the same frames;
    the first plan of each mode is also held against the operator on its own twin's macros."""
    tw = twin_macros(lambda: lbm.Context(NX, NY, options=PLANS[plans[0]], **KW), POINTS)
    base = None
    for plan in plans:
        frames = run_frames(lambda: lbm.Context(NX, NY, options=PLANS[plan], **KW), 4)
        assert [t for t, _ in frames] == POINTS
        if base is None:
            base = frames
            for t, f in frames:
                check(f, reference_frame(tw[t], 4), f"{plan} t={t}")
        for (t, f), (_, g) in zip(frames, base):
            assert np.array_equal(f, g), (plan, t)


def test_a_run_repeats_its_frames_bit_for_bit(lbm):
    make = lambda: lbm.Context(NX, NY, options=PLANS["fast-rowil-col6"], **KW)
    a, b = run_frames(make, 8), run_frames(make, 8)
    assert len(a) == 3 and all(np.array_equal(f, g) and t == u for (t, f), (u, g) in zip(a, b))


# ---- 3. strips ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("nstrips", [2, 3])
def test_a_group_of_strips_gives_the_whole_domains_frames(lbm, nstrips, k):
    """320x96 in strips of 48 / 32 rows: the coarse rows next to a strip face take d ux/dy from the ghost row, and that row's outlet
    cell pulls from the ghost row beyond it."""
    nx, ny, kw = 320, 96, dict(inlet_velocity=0.06, cylinder_radius=0.12)
    plan = PLANS["rowil-deep6-nt"]
    whole = run_frames(lambda: lbm.Context(nx, ny, options=plan, **kw), k, calls=((5, 45), (130, 45)))
    with lbm.Group(nx, ny, nstrips, options=plan, **kw) as g:
        g.initialise()
        g.frames_begin(k)
        g.step(5, 45)
        g.step(130, 45)
        assert g.first_unstable_step() == -1 and g.frames_pending() == 3
        got = g.drain_frames()
        assert g.frames_pending() == 0
    assert [t for t, _ in got] == [t for t, _ in whole] == [0, 45, 90]
    for (t, f), (_, w) in zip(got, whole):
        assert f.shape == (4, ny // k, nx // k)
        assert np.array_equal(f, w), (t, np.argwhere(f != w)[:8])
    assert np.max(np.abs(whole[-1][1][3])) > 1e-4


def test_the_frames_keyword_begins_frames_on_every_member(lbm):
    with lbm.Group(320, 96, 2, frames=8, inlet_velocity=0.06) as g:
        g.initialise()
        g.step(3, 2)
        got = g.drain_frames()
    assert [t for t, _ in got] == [0, 2] and got[0][1].shape == (4, 12, 40)


# ---- 4. frames change nothing else --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-deep6-nt", "fast-rowil-col6"])
def test_frames_change_reporting_only(lbm, plan):
    def run(frames):
        with lbm.Context(NX, NY, options=PLANS[plan], frames=frames, **KW) as c:
            c.initialise()
            c.step(STEPS, OF)
            return c.populations("f_next"), c.macros(), c.drain_force_log(), c.kernel_name(), c.plan_options() if plan != "auto" else None
    a, b = run(None), run(4)
    assert np.array_equal(a[0], b[0])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert a[2] == b[2] and len(a[2]) == 3
    assert a[3] == b[3] and a[4] == b[4]


# ---- 5. fp32 contexts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
def test_fp32_contexts_average_their_own_macros_in_double(lbm, k):
    frames = run_frames(lambda: lbm.Context(NX, NY, precision="f32", options=F32_PLAN, **KW), k)
    tw = twins(lbm, "disc", "f32")
    assert [t for t, _ in frames] == POINTS
    for t, f in frames:
        check(f, reference_frame(tw[t], k), f"fp32 k={k} t={t}")
    assert np.max(np.abs(frames[-1][1][3])) > 1e-4


# ---- 6. the ring --------------------------------------------------------------------------------------------------------------------
def test_the_ring_fills_drains_oldest_first_and_resets(lbm):
    with lbm.Context(NX, NY, **KW) as c:
        c.initialise()
        assert c.drain_frames() == [] and c.frames_pending() == 0          # never begun
        c.frames_begin(8, capacity=2)
        c.step(10, 5)                                                      # t = 0, 5 fill the ring; t = 10 finds it full
        assert c.frames_pending() == 2
        with pytest.raises(lbm.LbmError, match="drain"):
            c.step(1, 5)
        assert c.steps_done == 10 and c.frames_pending() == 2
        first = c.drain_frames(1)
        assert [t for t, _ in first] == [0] and c.frames_pending() == 1
        c.step(1, 5)                                                       # t = 10 goes into the slot that was freed (the ring wraps)
        assert c.frames_pending() == 2
        rest = c.drain_frames()
        assert [t for t, _ in rest] == [5, 10] and c.frames_pending() == 0
        assert not np.array_equal(rest[0][1], rest[1][1])
        c.step(5, 5)                                                       # t = 15
        c.frames_end()
        c.step(5, 5)                                                       # t = 20: not sampled
        assert c.frames_pending() == 1
        c.frames_begin(8, capacity=2)                                      # again: the ring is empty
        assert c.frames_pending() == 0 and c.drain_frames() == []
        c.step(5, 5)                                                       # t = 25
        assert [t for t, _ in c.drain_frames()] == [25]
        # the frames of t = 0 and of the wrapped slot are what a fresh run gives
    again = run_frames(lambda: lbm.Context(NX, NY, **KW), 8, calls=((11, 5),), capacity=4)
    assert np.array_equal(again[0][1], first[0][1]) and np.array_equal(again[2][1], rest[1][1])


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_named(lbm):
    L = lbm.lib()
    err = lambda: L.lbm_last_error().decode()
    assert L.lbm_frames_begin(None, 4, 2) == -1 and "initialised context" in err()
    assert L.lbm_frames_end(None) == -1 and L.lbm_frames_pending(None) == -1 and L.lbm_drain_frames(None, None, None, 1) == -1
    with lbm.Context(NX, NY, **KW) as c:
        assert L.lbm_frames_begin(c.h, 4, 2) == -1 and "initialised context" in err()
        c.initialise()
        for k, text in [(0, "k = 0 outside 1..64"), (65, "k = 65 outside 1..64"), (5, "does not divide nx = 192")]:
            assert L.lbm_frames_begin(c.h, k, 2) == -1 and text in err(), (k, err())
        assert L.lbm_frames_begin(c.h, 4, 0) == -1 and "capacity 0" in err()
        with pytest.raises(lbm.LbmError, match="frames"):
            c.set_option("frames", 65)
        assert c.frames_pending() == 0
        c.step(2, 1)
        assert c.drain_frames() == []
    with lbm.Context(NX, NY, y_start=16, local_ny=24, **KW) as c:      # a strip of 24 rows from row 16
        c.initialise()
        assert L.lbm_frames_begin(c.h, 16, 2) == -1 and "local_ny = 24" in err()
        assert L.lbm_frames_begin(c.h, 3, 2) == -1 and "y_start = 16" in err()
        assert L.lbm_frames_begin(c.h, 8, 2) == 0


# ---- 8. lbm_solver --frame-stride ---------------------------------------------------------------------------------------------------
def read_frame_vtk(path):
    text = open(path).read()
    dims = [int(v) for v in re.search(r"DIMENSIONS (\d+) (\d+) 1", text).groups()]
    spacing = re.search(r"SPACING (\d+) (\d+) 1", text).groups()
    n = dims[0] * dims[1]
    vel = np.array(text.split("VECTORS velocity float\n")[1].split("\n\n")[0].split(), dtype=np.float64).reshape(n, 3)
    rho = np.array(text.split("SCALARS density float\nLOOKUP_TABLE default\n")[1].split("\n\n")[0].split(), dtype=np.float64)
    w = np.array(text.split("SCALARS vorticity float\nLOOKUP_TABLE default\n")[1].split(), dtype=np.float64)
    shape = (dims[1], dims[0])
    return np.stack([rho.reshape(shape), vel[:, 0].reshape(shape), vel[:, 1].reshape(shape), w.reshape(shape)]), spacing


@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]], ids=["whole", "three-strips"])
def test_lbm_solver_writes_the_bindings_frames(lbm, tmp_path, extra):
    base = [EXE, "--nx", "128", "--ny", "48", "--steps", "201", "--output-frequency", "100", "--no-vtk", "--no-tune", "--quiet"] + extra
    with_frames, without = tmp_path / "a", tmp_path / "b"
    for d, args in ((with_frames, ["--frame-stride", "4"]), (without, [])):
        d.mkdir()
        r = subprocess.run(base + args, cwd=d, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
    names = sorted(os.listdir(with_frames / "vtk_output"))
    assert names == ["frame_000000.vtk", "frame_000100.vtk", "frame_000200.vtk"]
    assert not (without / "vtk_output").exists()
    with lbm.Context(128, 48, options=dict(tune=0)) as c:      # the solver's defaults (LBM::SimulationParams) are the binding's
        c.initialise()
        c.frames_begin(4)
        c.step(201, 100)
        frames = dict(c.drain_frames())
    for t in (0, 100, 200):
        got, spacing = read_frame_vtk(with_frames / "vtk_output" / f"frame_{t:06d}.vtk")
        assert spacing == ("4", "4") and got.shape == (4, 12, 32)
        assert np.max(np.abs(got - frames[t].astype(np.float64))) <= 0.5e-8 + 1e-15, t      # "%.8f"
    assert np.max(np.abs(frames[200][3])) > 1e-4
    for name in ("forces.csv", "velocity_field.csv"):
        assert open(with_frames / name).read() == open(without / name).read()
    a, b = open(with_frames / "simulation_params.csv").read(), open(without / "simulation_params.csv").read()
    assert a == b + "frame_stride,4\n"
