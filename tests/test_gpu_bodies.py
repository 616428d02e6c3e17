"""Momentum-exchange forces per obstacle body (lbm_set_body_labels, Context(bodies=...), Group(bodies=...), lbm_solver --obstacle-bodies)
on the GPU.

The reference for every comparison is numpy, below: `link_forces` of tests/reference.py with the selection "fluid cell (label 0)
whose neighbour carries label k", applied to the post-collision populations P_t the kernel itself read. The device holds P_t in
buf[cur] at steps_done == t and hands it out as populations("f_next") once steps_done == t + 1 (include/lbm_hip.h, time convention), so
every sample point t is driven as: step to t, read body_forces() and forces(), step(1, of) — which logs row t — and read
populations("f_next") == P_t of the same context. Only the new kernel is under test; fp32 populations arrive as doubles.

The bar is 1e-13 * max(1, sum |2 c_i f_i|) per component, the sum running over the links of that body (of all bodies for a total):
both sides add the same addends in tree order, error O(log N * 2^-53 * sum |a|) ~ 1e-15 * sum |a|; 1e-13 is the project's
strips-against-whole figure."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import EXE, PLANS, lbm_gpu, read_params, write_pgm  # noqa: F401
from tests.reference import CX, CY

pytestmark = pytest.mark.gpu
NX, NY, STEPS, OF = 192, 64, 120, 30
# {planar, row-interleaved} x {fp64, fp32} of tests.helpers.PLANS, and one register-kernel plan (k_stepc_col)
CONFIGS = {"planar-f64": ("planar-site", "f64"), "planar-f32": ("planar-site", "f32"), "rowil-f64": ("rowil-site-nt", "f64"),
           "rowil-f32": ("rowil-site-nt", "f32"), "register-f64": ("rowil-col5-nt", "f64")}


def shifted(a, i):
    """nb[y, x] = a[y + cy_i, x + cx_i] where that neighbour lies in the domain, else 0."""
    ny, nx = a.shape
    nb = np.zeros_like(a)
    ys, yd = (slice(CY[i], None), slice(0, ny - CY[i])) if CY[i] >= 0 else (slice(0, ny + CY[i]), slice(-CY[i], None))
    xs, xd = (slice(CX[i], None), slice(0, nx - CX[i])) if CX[i] >= 0 else (slice(0, nx + CX[i]), slice(-CX[i], None))
    nb[yd, xd] = a[ys, xs]
    return nb


def body_link_forces(f_next, labels, k, rows=None):
    """(fx, fy, sum |2 cx f|, sum |2 cy f|) over the links fluid cell x -> neighbour x + c_i of label k (k None: any nonzero label),
    fluid cells in the global rows [rows[0], rows[1]) only (a strip's partial sum); f_next ghost-inclusive, whole domain."""
    f = f_next[1:-1, 1:-1]
    fx = fy = ax = ay = 0.0
    for i in range(1, 9):
        nb = shifted(labels, i)
        sel = ((nb != 0) if k is None else (nb == k)) & (labels == 0)
        if rows is not None:
            sel[:rows[0]] = False
            sel[rows[1]:] = False
        v = f[..., i][sel]
        s, a = float(np.sum(v)), float(np.sum(np.abs(v)))
        fx += 2.0 * CX[i] * s; fy += 2.0 * CY[i] * s
        ax += 2.0 * abs(CX[i]) * a; ay += 2.0 * abs(CY[i]) * a
    return fx, fy, ax, ay


def within(got, want, scale):
    return abs(got - want) <= 1e-13 * max(1.0, scale)


def disc(lab, cx, cy, r, k):
    y, x = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    lab[(x - cx) ** 2 + (y - cy) ** 2 <= r * r] = k
    return lab


def label_sets(nx=NX, ny=NY):
    z = lambda: np.zeros((ny, nx), np.uint8)
    out = {"tandem": disc(disc(z(), 50, 32, 6, 1), 90, 32, 6, 2)}
    m = z(); m[24:40, 60:76] = 1; m[24:40, 76:92] = 2
    out["touching"] = m
    m = z(); m[0:10, 100:116] = 1; m[20:30, 0:1] = 2; m[40:50, 191:192] = 3
    out["walls"] = m
    out["gap"] = disc(disc(z(), 50, 32, 6, 1), 90, 32, 6, 3)
    out["single"] = disc(disc(z(), 50, 32, 6, 1), 90, 32, 6, 1)
    return out


SETS = label_sets()


def drive(ctx, steps, of, first=0):
    """Steps ctx from `first` to `steps` so that every sample point t (t % of == 0) is visited as described in the module docstring.
    Returns [(t, body_forces() (B, 2), forces(), P_t)]."""
    out = []
    t = first
    while t < steps:
        if t % of == 0:
            bf, tot = ctx.body_forces(), ctx.forces()
            ctx.step(1, of)
            out.append((t, bf, tot, ctx.populations("f_next")))
            t += 1
        else:
            n = min(steps, (t // of + 1) * of) - t
            ctx.step(n, of)
            t += n
    assert ctx.steps_done == steps and ctx.first_unstable_step() == -1
    return out


def check_against_numpy(labels, samples, log, blog, rows=None):
    """Every logged row and every body_forces() row against numpy on P_t; the sum over the bodies against the logged total."""
    B = int(labels.max())
    assert [t for t, _, _ in log] == [t for t, _, _, _ in samples]
    assert [(t, b) for t, b, _, _ in blog] == [(t, b) for t, _, _ in log for b in range(1, B + 1)]
    for n, (t, bf, tot, pt) in enumerate(samples):
        assert bf.shape == (B, 2)
        sx = sy = 0.0
        for k in range(1, B + 1):
            rx, ry, ax, ay = body_link_forces(pt, labels, k, rows)
            _, _, lx, ly = blog[n * B + k - 1]
            print(f"t={t} body {k}: log ({lx:.17g}, {ly:.17g}) now ({bf[k - 1, 0]:.17g}, {bf[k - 1, 1]:.17g}) numpy ({rx:.17g}, {ry:.17g}) "
                  f"err ({abs(lx - rx):.2e}, {abs(ly - ry):.2e}) bar ({1e-13 * max(1, ax):.2e}, {1e-13 * max(1, ay):.2e})")
            assert within(lx, rx, ax) and within(ly, ry, ay), (t, k)
            assert bf[k - 1, 0] == lx and bf[k - 1, 1] == ly, (t, k)        # the same kernel on the same P_t: the same bits
            sx += lx; sy += ly
        tx, ty, ax, ay = body_link_forces(pt, labels, None, rows)
        assert within(sx, log[n][1], ax) and within(sy, log[n][2], ay), t
        assert within(log[n][1], tx, ax) and within(log[n][2], ty, ay), t
        assert tot == (log[n][1], log[n][2])


# ---- 1-3. rows against numpy; gap; single == total; bodies add up to the total ---------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", list(SETS))
def test_rows_meet_the_numpy_reference(lbm, name, config):
    plan, prec = CONFIGS[config]
    labels = SETS[name]
    with lbm.Context(NX, NY, tau=0.6, options=PLANS[plan], precision=prec, bodies=labels) as ctx:
        assert ctx.initialise() == int((labels != 0).sum()) and ctx.body_count() == int(labels.max())
        if config == "register-f64":
            assert "k_stepc_col" in ctx.kernel_name()
        samples = drive(ctx, STEPS, OF)
        log, blog = ctx.drain_force_log(), ctx.drain_body_force_log()
    assert [t for t, _, _ in log] == [0, 30, 60, 90]
    check_against_numpy(labels, samples, log, blog)
    if name == "gap":
        rows2 = [r for r in blog if r[1] == 2]
        assert len(rows2) == 4 and all(r[2] == 0.0 and r[3] == 0.0 for r in rows2)
        assert all(np.array_equal(bf[1], [0.0, 0.0]) for _, bf, _, _ in samples)
    if name == "single":
        assert np.array_equal(np.array([r[2:] for r in blog]), np.array([r[1:] for r in log]))
        for (t, bf, tot, _) in samples:
            assert np.array_equal(bf[0], np.array(tot))


# ---- 4. labels change reporting only ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS))
def test_labels_leave_everything_else_as_the_mask_leaves_it(lbm, config):
    plan, prec = CONFIGS[config]
    labels = SETS["tandem"]
    runs = []
    for kw in (dict(solid=labels != 0), dict(bodies=labels)):
        with lbm.Context(NX, NY, tau=0.6, options=PLANS[plan], precision=prec, **kw) as ctx:
            n = ctx.initialise()
            ctx.step(STEPS, OF)
            runs.append((n, ctx.populations("f_next"), ctx.populations("f_current"), ctx.macros(), ctx.drain_force_log(), ctx.kernel_name(),
                         ctx.solid(), ctx.forces(), ctx.body_count(), len(ctx.drain_body_force_log())))
    a, b = runs
    assert a[0] == b[0] and a[4] == b[4] and a[5] == b[5] and a[7] == b[7] and len(a[4]) == 4
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[6], b[6])
    for u, v in zip(a[3], b[3]):
        assert np.array_equal(u, v)
    assert (a[8], a[9]) == (0, 0) and (b[8], b[9]) == (2, 8)


# ---- 5. strips --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["rowil-site-nt", "rowil-col5-nt"])
@pytest.mark.parametrize("nstrips", [2, 3])
@pytest.mark.parametrize("name", ["tandem", "walls"])
def test_group_strips(lbm, name, nstrips, plan):
    """ny = 64 in two strips puts the boundary (row 32) through both tandem discs; in three strips (22 + 21 + 21 rows) the discs and
    their dilated boxes (rows 25..39) lie in the middle strip, and the walls set's bodies 1 / 3 are out of reach of the top / bottom strip."""
    labels = SETS[name]
    B = int(labels.max())
    with lbm.Context(NX, NY, tau=0.6, options=PLANS[plan], bodies=labels) as whole:
        solid = whole.initialise()
        whole.step(STEPS, OF)
        w = (whole.populations("f_next"), whole.drain_force_log(), whole.drain_body_force_log(), whole.body_forces())
    with lbm.Group(NX, NY, nstrips, options=PLANS[plan], tau=0.6, bodies=labels) as g:
        assert g.initialise() == solid and g.body_count() == B
        samples = drive(g, STEPS, OF)
        assert np.array_equal(g.populations("f_next"), w[0])
        now = g.body_forces()
        parts = [c.drain_body_force_log() for c in g.ctxs]
        bounds = [(c.y_start, c.y_start + c.local_ny) for c in g.ctxs]
        log = g.drain_force_log()
    assert len(w[2]) == 4 * B and all(len(p) == 4 * B for p in parts)
    # every strip's partial sums against numpy on the rows it owns; a strip out of a body's reach reports exact zeros
    for (y0, y1), part in zip(bounds, parts):
        for n, (t, _, _, pt) in enumerate(samples):
            for k in range(1, B + 1):
                rx, ry, ax, ay = body_link_forces(pt, labels, k, (y0, y1))
                _, body, fx, fy = part[n * B + k - 1]
                assert body == k and within(fx, rx, ax) and within(fy, ry, ay), (y0, t, k)
                ys = np.nonzero((labels == k).any(axis=1))[0]
                if ys.max() + 1 < y0 or ys.min() - 1 >= y1:
                    assert fx == 0.0 and fy == 0.0, (y0, t, k)
    if nstrips == 3:
        zero = {"tandem": [(0, 1), (0, 2), (2, 1), (2, 2)], "walls": [(1, 1), (2, 1), (0, 3), (2, 2)]}[name]
        for s, k in zero:
            assert all(r[2] == 0.0 and r[3] == 0.0 for r in parts[s] if r[1] == k), (s, k)
    # the strips' rows summed per (t, body) against the whole context's
    for n, (t, k, wx, wy) in enumerate(w[2]):
        _, _, ax, ay = body_link_forces(samples[n // B][3], labels, k)
        sx, sy = sum(p[n][2] for p in parts), sum(p[n][3] for p in parts)
        assert (parts[0][n][0], parts[0][n][1]) == (t, k) and within(sx, wx, ax) and within(sy, wy, ay), (t, k)
    assert [r[0] for r in log] == [r[0] for r in w[1]]
    for k in range(B):
        _, _, ax, ay = body_link_forces(w[0], labels, k + 1)
        assert within(now[k, 0], w[3][k, 0], ax) and within(now[k, 1], w[3][k, 1], ay)


def test_group_log_sums_the_strips_in_strip_order(lbm):
    labels = SETS["tandem"]
    with lbm.Group(NX, NY, 2, options=PLANS["rowil-site-nt"], tau=0.6, bodies=labels) as a, \
            lbm.Group(NX, NY, 2, options=PLANS["rowil-site-nt"], tau=0.6, bodies=labels) as b:
        for g in (a, b):
            g.initialise()
            g.step(61, 30)
        parts = [c.drain_body_force_log() for c in a.ctxs]
        merged = b.drain_body_force_log()
    assert len(merged) == 6 and merged == [(p[0], p[1], 0 + p[2] + q[2], 0 + p[3] + q[3]) for p, q in zip(*parts)]


# ---- 6. a box of more than one chunk ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["rowil-f64", "planar-f32", "register-f64"])
def test_a_box_of_several_chunks(lbm, config):
    plan, prec = CONFIGS[config]
    nx, ny, steps, of = 512, 160, 60, 20
    y, x = np.mgrid[0:ny, 0:nx]
    labels = np.zeros((ny, nx), np.uint8)
    labels[(x % 16 == 8) & (y % 16 == 8)] = 1
    disc(labels, 100, 80, 8, 2)
    _, boxes, chunks = lbm.debug_body_chunks(labels)
    assert (boxes[0, 1] - boxes[0, 0] + 1) * (boxes[0, 3] - boxes[0, 2] + 1) > 65536 and chunks[:, 0].tolist() == [1, 1, 2]
    runs = []
    for rep in range(2):
        with lbm.Context(nx, ny, tau=0.6, options=PLANS[plan], precision=prec, bodies=labels) as ctx:
            ctx.initialise()
            if rep == 0:
                samples = drive(ctx, steps, of)
            else:
                ctx.step(steps, of)
            runs.append((ctx.drain_force_log(), ctx.drain_body_force_log()))
    assert [t for t, _, _ in runs[0][0]] == [0, 20, 40]
    check_against_numpy(labels, samples, *runs[0])
    assert runs[0] == runs[1]          # identical bits, whatever the launch sequence that led to P_t


# ---- 7. checkpoints ---------------------------------------------------------------------------------------------------------
def test_checkpoints_are_those_of_the_mask(lbm, tmp_path):
    labels = SETS["touching"]
    opts = PLANS["rowil-site-nt"]
    with lbm.Context(NX, NY, tau=0.6, options=opts, bodies=labels) as u:
        u.initialise()
        u.step(60, 25)
        u.drain_force_log(); u.drain_body_force_log()
        u.step(50, 25)
        ref = (u.populations("f_next"), u.drain_force_log(), u.drain_body_force_log())
    with lbm.Context(NX, NY, tau=0.6, options=opts, bodies=labels) as a:
        a.initialise()
        a.step(60, 25)
        a.save_state(tmp_path / "bodies.ckpt")
    with lbm.Context(NX, NY, tau=0.6, options=opts, solid=labels != 0) as s:
        s.initialise()
        s.step(60, 25)
        s.save_state(tmp_path / "solid.ckpt")
    fb, fs = open(tmp_path / "bodies.ckpt", "rb").read(), open(tmp_path / "solid.ckpt", "rb").read()
    assert fb[:8] == fs[:8] == b"LBMCKPT2"
    assert fb == fs                     # labels are not in the file: byte for byte the mask's checkpoint
    for kw in (dict(solid=labels != 0), dict(bodies=labels)):
        with lbm.Context(NX, NY, tau=0.6, options=opts, **kw) as b:
            b.initialise()
            b.load_state(tmp_path / "bodies.ckpt")
            assert b.steps_done == 60
            b.step(50, 25)
            assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
            blog = b.drain_body_force_log()
            assert blog == (ref[2] if "bodies" in kw else [])
    assert [r[0] for r in ref[1]] == [75, 100] and len(ref[2]) == 4


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------
def test_arguments(lbm):
    import ctypes as C
    labels = SETS["tandem"]
    ub = C.POINTER(C.c_ubyte)
    raw = np.ascontiguousarray(labels)
    with pytest.raises(lbm.LbmError):
        lbm.Context(NX, NY, solid=labels != 0, bodies=labels)
    with lbm.Context(NX, NY, tau=0.6, options=PLANS["planar-site"]) as ctx:
        # null pointer and wrong dimensions, as lbm_set_solid_mask refuses them
        assert ctx.L.lbm_set_body_labels(ctx.h, None, NX, NY) == -1
        assert ctx.L.lbm_set_body_labels(ctx.h, raw.ctypes.data_as(ub), NX - 1, NY) == -1
        assert ctx.L.lbm_set_body_labels(ctx.h, raw.ctypes.data_as(ub), NX, NY + 1) == -1 and b"lbm_set_body_labels" in ctx.L.lbm_last_error()
        assert ctx.body_count() == 0
        ctx.set_body_labels(labels)
        assert ctx.body_count() == 2
        ctx.set_solid_mask(labels != 0)          # a later mask clears the labels
        assert ctx.body_count() == 0
        ctx.initialise()
        with pytest.raises(lbm.LbmError, match="before lbm_initialise"):
            ctx.set_body_labels(labels)
        ctx.step(2, 1)
        with pytest.raises(lbm.LbmError, match="error -1.*no body labels"):
            ctx.body_forces()
        assert ctx.drain_body_force_log() == []
    with lbm.Context(NX, NY, tau=0.6, options=PLANS["planar-site"], bodies=SETS["single"]) as ctx:
        ctx.set_body_labels(SETS["walls"])       # a later call replaces mask and labels
        assert ctx.body_count() == 3 and ctx.initialise() == int((SETS["walls"] != 0).sum())
        assert np.array_equal(ctx.solid(), SETS["walls"] != 0)
        ctx.step(4, 1)
        assert ctx.drain_body_force_log(max_rows=2) == []          # fewer rows than one sample: nothing is copied
        first = ctx.drain_body_force_log(max_rows=7)               # whole samples only: two of them
        assert [(r[0], r[1]) for r in first] == [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]
        rest = ctx.drain_body_force_log()
        assert [(r[0], r[1]) for r in rest] == [(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3)]
        assert ctx.drain_body_force_log() == []


def test_the_log_is_a_ring_of_force_log_capacity_samples(lbm):
    labels = SETS["tandem"]
    with lbm.Context(NX, NY, tau=0.6, options=PLANS["planar-site"], bodies=labels) as ref:
        ref.initialise()
        ref.step(5, 1)
        want = ref.drain_body_force_log()
    with lbm.Context(NX, NY, tau=0.6, options=PLANS["planar-site"], bodies=labels, force_log_capacity=3) as ctx:
        ctx.initialise()
        ctx.step(3, 1)
        with pytest.raises(lbm.LbmError, match="log full"):
            ctx.step(1, 1)
        assert len(ctx.drain_force_log()) == 3
        with pytest.raises(lbm.LbmError, match="body force log full"):
            ctx.step(1, 1)
        got = ctx.drain_body_force_log(max_rows=2)      # one sample leaves; the next one wraps into its slot
        ctx.step(1, 1)
        got += ctx.drain_body_force_log()
        ctx.drain_force_log()
        ctx.step(1, 1)
        got += ctx.drain_body_force_log()
    assert got == want and len(got) == 10


# ---- 9. lbm_solver --obstacle-bodies ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
def test_lbm_solver_writes_forces_per_body(lbm, tmp_path, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    labels = disc(disc(np.zeros((ny, nx), np.uint8), 50, 24, 6, 1), 90, 24, 6, 2)
    write_pgm(tmp_path / "bodies.pgm", labels)
    base = [EXE, "--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--no-vtk", "--no-tune"] + extra
    outs = {}
    for flag in ("--obstacle-bodies", "--obstacle-mask"):
        d = tmp_path / flag.strip("-")
        d.mkdir()
        r = subprocess.run(base + [flag, str(tmp_path / "bodies.pgm")], cwd=d, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        outs[flag] = (d, r.stdout)
    db, banner = outs["--obstacle-bodies"]
    dm, _ = outs["--obstacle-mask"]
    assert open(db / "forces.csv", "rb").read() == open(dm / "forces.csv", "rb").read()
    assert open(db / "velocity_field.csv", "rb").read() == open(dm / "velocity_field.csv", "rb").read()
    assert not os.path.exists(dm / "forces_bodies.csv")
    cells = int((labels == 1).sum())
    assert f"Body 1: {cells} cells, D=13" in banner and f"Body 2: {cells} cells, D=13" in banner, banner
    params = read_params(db / "simulation_params.csv")
    assert params["obstacle_bodies"] == str(tmp_path / "bodies.pgm") and params["body_count"] == "2" and "obstacle_mask" not in params
    lines = open(db / "forces_bodies.csv").read().splitlines()
    assert lines[0] == "timestep,body,drag_force,lift_force,drag_coeff,lift_coeff"
    rows = [l.split(",") for l in lines[1:]]
    with lbm.Context(nx, ny, bodies=labels) as ctx:       # (the defaults of the binding are those of the command line)
        ctx.initialise()
        ctx.step(steps, of)
        assert ctx.first_unstable_step() == -1
        blog = ctx.drain_body_force_log()
    assert [(int(r[0]), int(r[1])) for r in rows] == [(t, b) for t, b, _, _ in blog] == [(t, b) for t in (0, 100, 200, 300) for b in (1, 2)]
    q = 0.5 * 0.01333 * 0.01333 * 13
    for r, (t, b, fx, fy) in zip(rows, blog):
        for got, want in zip(map(float, r[2:4]), (fx, fy)):
            assert abs(got - want) <= 1.5e-8, (t, b, r)
        for got, want in zip(map(float, r[4:6]), (fx / q, fy / q)):
            assert abs(got - want) <= 1.5e-8, (t, b, r)
