"""Per-row inlet velocity profiles (lbm_set_inlet_profile, Context/Group(inlet_profile=...), lbm_solver --inlet-profile) on the GPU.

The reference's Zou-He inlet with u_in replaced by u[y] on row y, and an initial state of f_eq(1, (u[y], 0)) per row. The oracle
imposes one velocity; its arrays are writable views, so the stepwise oracle with the numpy boundary step (oracle_run(u=...) of
tests/reference.py, in the oracle's operation order) is the per-row reference: strict plans must match it bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PLANS, TALL_F32, assert_group_is_whole, assert_matches_reference, assert_same_results,  # noqa: F401
                           host_staged_two_strips, lbm_gpu, masks, read_csv_rows, read_params, read_velocity_field, record, run_ctx, run_solver,
                           square, strict, u_bar_rel, whole_run, write_pgm)
from tests.reference import oracle_run

pytestmark = pytest.mark.gpu


def shear(ny, mean):
    s = (np.arange(ny) + 1.0) / ny
    return s * (mean / np.mean(s))


def reversed_near_bottom(ny, mean):
    s = (np.arange(ny) + 0.5) / ny
    u = s * (1 - s)
    u[:8] = -0.6 * u[:8] - 0.002          # back-flow over the bottom eight rows (the inlet-outlet mask blocks rows 10..20 of x = 0)
    return u * (mean / np.mean(u))


# ---- 1. a constant profile is the uniform inlet, bit for bit -----------------------------------------------------------------
CONST_CASES = [(p, "f64", None) for p in PLANS] + [("tall-f32", "f32", None), ("col5-f32", "f32", None), ("rowil-col5-nt", "f64", "square"),
                                                   ("fast-rowil-col6", "f64", "square"), ("rowil-site-nt", "f32", "square")]


@pytest.mark.parametrize("plan,precision,mask", CONST_CASES, ids=["-".join(str(v) for v in c) for c in CONST_CASES])
def test_constant_profile_is_the_uniform_inlet(lbm, plan, precision, mask):
    nx, ny, steps, of = 1000, 200, 23, 7       # (1000 % 64 != 0: ragged last tiles)
    u0 = 0.05
    kw = dict(inlet_velocity=u0, cylinder_radius=0.08, precision=precision)
    opts = TALL_F32 if plan == "tall-f32" else PLANS["rowil-col5-nt"] if plan == "col5-f32" else PLANS[plan]
    solid = square(nx, ny) if mask else None
    a = run_ctx(lbm, nx, ny, opts, steps, of, solid=solid, **kw)
    b = run_ctx(lbm, nx, ny, opts, steps, of, solid=solid, inlet_profile=np.full(ny, u0), **kw)
    assert_same_results(a, b)


# ---- 2. non-uniform profiles against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["parabolic", "shear", "reversed-inlet-outlet"])
def test_profiles_against_the_oracle(lbm, name):
    nx, ny, steps, of = 200, 64, 60, 20        # (200 % 64 != 0: a ragged last tile column)
    kw = dict(inlet_velocity=0.05)
    mask = None
    if name == "parabolic":
        u = lbm.parabolic_profile(ny, 0.05)
    elif name == "shear":
        u = shear(ny, 0.05)
    else:
        u = reversed_near_bottom(ny, 0.05)
        mask = masks(nx, ny)["inlet-outlet"]
        assert np.min(u) < 0
    ref = oracle_run(nx, ny, steps, of, mask=mask, u=u, **kw)
    assert ref.first_unstable == -1
    fluid0 = np.ones(ny, bool) if mask is None else mask[:, 0] == 0
    assert np.array_equal(ref.ux[fluid0, 0], u[fluid0])
    seen = {}
    for plan in ORACLE_PLANS:
        with lbm.Context(nx, ny, options=PLANS[plan], solid=mask, inlet_profile=u, **kw) as ctx:
            ctx.initialise()
            rho0, ux0, uy0 = ctx.macros()         # the initial snapshot: ux = u[y] on every fluid cell
            sol = ctx.solid().astype(bool)
            assert np.array_equal(ux0[~sol], np.broadcast_to(u[:, None], (ny, nx))[~sol])
            ctx.step(steps, of)
            assert ctx.first_unstable_step() == -1
            log = ctx.drain_force_log()
            fn = ctx.populations("f_next")
            macros = ctx.macros()
        assert np.array_equal(macros[1][fluid0, 0], u[fluid0]), plan       # the inlet column reports u[y]
        key = "strict" if strict(plan) else "fast"
        seen.setdefault(key, fn)
        assert np.array_equal(fn, seen[key]), plan      # every plan of one arithmetic mode: the same bits
        assert_matches_reference(plan, fn, macros, log, ref, u_bar_rel(ref), fast_rho=False)


# ---- 3. strips ---------------------------------------------------------------------------------------------------------------
def wavy(ny, mean):
    """A profile whose every row differs from its neighbours (so every strip face sees a non-trivial inlet on both sides)."""
    y = np.arange(ny)
    s = (y + 0.5) / ny
    u = s * (1 - s) * (1.0 + 0.3 * np.sin(1.7 * y))
    return u * (mean / np.mean(u))


@pytest.mark.parametrize("nstrips", [3, 4])
@pytest.mark.parametrize("plan", ["rowil-col5-nt", "rowil-fuse3-12-nt-xcd"])
def test_group_strips_with_a_profile(lbm, plan, nstrips):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(inlet_velocity=0.06)
    u = wavy(ny, 0.06)
    w = whole_run(lbm, nx, ny, plan, steps, of, inlet_profile=u, **kw)
    with lbm.Group(nx, ny, nstrips, options=PLANS[plan], inlet_profile=u, **kw) as g:
        g.initialise()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)


@pytest.mark.parametrize("plan", [None, "rowil-col5-nt"])
def test_host_staged_strips_with_a_profile(lbm, plan):
    nx, ny = 512, 256
    kw = dict(inlet_velocity=0.05)
    u = wavy(ny, 0.05)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], inlet_profile=u, **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, _ = host_staged_two_strips(lbm, nx, ny, 12, 4, PLANS[plan] if plan else None, inlet_profile=u, **kw)
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 4. fp32 -----------------------------------------------------------------------------------------------------------------
def test_fp32_profiled_run_against_fp64(lbm):
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.05)
    u = lbm.parabolic_profile(ny, 0.05)
    with lbm.Context(nx, ny, inlet_profile=u, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", inlet_profile=u, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        m = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
    eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
    record("inlet_profile_fp32_vs_fp64", err_rho=er, err_u=eu)
    # the fp32 bars of tests/test_gpu_parity.py and test_gpu_thin_spots.py (rho 2e-5, u 2e-4): a uniform inlet measures rho 1.2e-5,
    # u 9.2e-5 after 1000 steps there; this profiled run measured rho 1.23e-5, u 1.05e-4 on MI355X
    assert er < 2e-5 and eu < 2e-4, (er, eu)
    assert np.array_equal(m[1][:, 0], u.astype(np.float32).astype(np.float64))   # the inlet column: (float)u[y]


# ---- 5. Poiseuille flow ------------------------------------------------------------------------------------------------------
def test_poiseuille_channel_reaches_the_parabola(lbm):
    nx, ny, tau, mean = 1024, 64, 0.8, 0.02
    nu = (tau - 0.5) / 3.0
    steps = int(4 * ny * ny / nu)
    u = lbm.parabolic_profile(ny, mean)
    empty = np.zeros((ny, nx), np.uint8)
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=mean, solid=empty, inlet_profile=u) as ctx:
        assert ctx.initialise() == 0
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        rho, ux, uy = ctx.macros()
    x = nx // 2
    y = np.arange(ny, dtype=np.float64)
    coef = np.polyfit(y, ux[:, x], 2)
    resid = float(np.max(np.abs(np.polyval(coef, y) - ux[:, x])) / np.max(ux[:, x]))
    uy_rel = float(np.max(np.abs(uy[:, x])) / mean)
    flux = [float(np.sum(rho[:, c] * ux[:, c])) for c in (0, nx // 4, x, 3 * nx // 4)]
    flux_err = abs(flux[2] - flux[0]) / abs(flux[0])                        # inlet (sum of rho_bc u[y]) against the middle
    flux_dev = max(abs(f - flux[2]) for f in flux[1:]) / abs(flux[2])        # along the developed channel
    record("inlet_profile_poiseuille", nx=nx, ny=ny, tau=tau, steps=steps, parabola_max_resid_rel=resid, uy_max_rel=uy_rel,
           mass_flux_rel_err=flux_err, mass_flux_developed_rel_err=flux_dev, ux_max=float(np.max(ux[:, x])), curvature=float(coef[0]))
    assert np.array_equal(ux[:, 0], u)
    assert coef[0] < 0
    assert resid <= 2e-3, resid
    assert uy_rel <= 1e-4, uy_rel
    assert flux_dev <= 2e-3, flux_dev
    # The inlet's sum of rho_bc u[y] is the momentum the Zou-He condition imposes on the inlet NODES, not the mass carried over the
    # links into the domain: the imposed parabola spans the ny rows while the developed one spans the ny - 1 cells between the wall
    # nodes (measured on MI355X: peak 0.02985 against 0.02999, the fitted zeros ~63 rows apart), and the entrance region between them
    # is not developed. Measured 2.9e-2 there; the bar only guards against a gross error.
    assert flux_err <= 5e-2, flux_err


# ---- 6. checkpoints ----------------------------------------------------------------------------------------------------------
def test_profiled_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.07)
    u = lbm.parabolic_profile(ny, 0.07)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], inlet_profile=u, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "p.ckpt")
        a.step(100, 50)
        ref = (a.populations("f_next"), a.drain_force_log())
    assert open(tmp_path / "p.ckpt", "rb").read(8) == b"LBMCKPT3"
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], inlet_profile=u, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "p.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    with lbm.Context(nx, ny, **kw) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="with an inlet profile; this context has none"):
            c.load_state(tmp_path / "p.ckpt")
        c.step(3, 0)
        c.save_state(tmp_path / "plain.ckpt")
    other = u.copy()
    other[5] += 1e-12
    with lbm.Context(nx, ny, inlet_profile=other, **kw) as d:
        d.initialise()
        with pytest.raises(lbm.LbmError, match="different inlet profile"):
            d.load_state(tmp_path / "p.ckpt")
        with pytest.raises(lbm.LbmError, match="without an inlet profile; this context has one"):
            d.load_state(tmp_path / "plain.ckpt")
    mask = square(nx, ny)
    with lbm.Context(nx, ny, solid=mask, **kw) as e:
        e.initialise()
        with pytest.raises(lbm.LbmError, match="with an inlet profile; this context has none"):
            e.load_state(tmp_path / "p.ckpt")
    # masked and profiled: both digests are checked
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, **kw) as f:
        f.initialise()
        f.step(11, 0)
        f.save_state(tmp_path / "mp.ckpt")
        f.load_state(tmp_path / "mp.ckpt")
        with pytest.raises(lbm.LbmError, match="without an obstacle mask"):
            f.load_state(tmp_path / "p.ckpt")
    with lbm.Context(nx, ny, solid=mask, inlet_profile=u, **kw) as g:
        g.initialise()
        g.load_state(tmp_path / "mp.ckpt")
        g.step(1, 0)
    other_mask = mask.copy()
    other_mask[3, 3] = 1
    with lbm.Context(nx, ny, solid=other_mask, inlet_profile=u, **kw) as h:
        h.initialise()
        with pytest.raises(lbm.LbmError, match="different obstacle mask"):
            h.load_state(tmp_path / "mp.ckpt")


# ---- 7. arguments ------------------------------------------------------------------------------------------------------------
def test_set_inlet_profile_arguments(lbm):
    nx, ny = 128, 32
    u = lbm.parabolic_profile(ny, 0.05)
    with lbm.Context(nx, ny) as ctx:
        L, dp = ctx.L, C.POINTER(C.c_double)

        def call(arr, n):
            a = np.ascontiguousarray(arr, dtype=np.float64)
            return L.lbm_set_inlet_profile(ctx.h, a.ctypes.data_as(dp), n)
        assert L.lbm_set_inlet_profile(ctx.h, None, ny) == -1 and b"null" in L.lbm_last_error()
        assert call(u, ny - 1) == -1 and b"rows given" in L.lbm_last_error()
        bad = u.copy(); bad[7] = np.nan
        assert call(bad, ny) == -1 and b"row 7" in L.lbm_last_error()
        bad = u.copy(); bad[0] = np.inf
        assert call(bad, ny) == -1 and b"row 0" in L.lbm_last_error()
        bad = u.copy(); bad[31] = 1.0
        assert call(bad, ny) == -1 and b"below 1" in L.lbm_last_error()
        assert call(u, ny) == 0
        ctx.initialise()
        assert call(u, ny) == -1 and b"before lbm_initialise" in L.lbm_last_error()
    with pytest.raises(lbm.LbmError):
        lbm.Context(nx, ny, inlet_profile=np.full(ny + 1, 0.01))


# ---- 8. the host CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--gpus", "1"], ["--gpus", "1", "--strips", "3"]])
@pytest.mark.parametrize("source", ["parabolic", "file"])
def test_lbm_solver_inlet_profile_matches_the_binding(lbm, tmp_path, source, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    mean = 0.04
    mask = np.zeros((ny, nx), np.uint8)
    mask[18:30, 30:42] = 1                    # square, frontal height D = 12
    write_pgm(tmp_path / "sq.pgm", mask * 255)
    if source == "parabolic":
        spec, u = "parabolic", lbm.parabolic_profile(ny, mean)
    else:
        shape = 1.0 + 0.5 * np.cos(np.arange(ny) * 0.3)
        (tmp_path / "shape.txt").write_text("# a shape\n" + "\n".join(repr(float(v)) for v in shape) + "\n")
        spec, u = str(tmp_path / "shape.txt"), lbm.scale_inlet_profile(shape, mean)
    pr = run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--inlet-velocity", str(mean),
                     "--no-vtk", "--obstacle-mask", str(tmp_path / "sq.pgm"), "--inlet-profile", spec] + extra, tmp_path)
    assert "Inlet: profile" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, inlet_velocity=mean, solid=mask, inlet_profile=u) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        log = ctx.drain_force_log()
        rho, ux, uy = ctx.macros()
    q = 0.5 * mean * mean * 12                # Cd / Cl refer to the mean (bulk) velocity
    assert [int(r[0]) for r in rows] == [t for t, _, _ in log]
    for r, (t, fx, fy) in zip(rows, log):
        for got, want in zip(map(float, r[1:]), (fx, fy, fx / q, fy / q)):
            assert abs(got - want) <= 1.5e-8, (t, r)
    cux, cuy, crho = read_velocity_field(tmp_path / "velocity_field.csv", nx, ny)
    assert np.max(np.abs(cux[:, 0] - u)) <= 5.1e-9           # the inlet column is the profile (8 decimals)
    for got, want in ((cux, ux), (cuy, uy), (crho, rho)):
        assert np.max(np.abs(got - want)) <= 5.1e-9
    params = read_params(tmp_path / "simulation_params.csv")
    assert params["inlet_profile"] == spec and params["obstacle_mask"].endswith("sq.pgm")
    assert abs(float(params["inlet_velocity"]) - mean) < 1e-12
    keys = list(params)
    assert keys.index("inlet_profile") == len(keys) - 1
