"""User-defined obstacle geometry (lbm_set_solid_mask, Context(solid=...), Group(solid=...), lbm_solver --obstacle-mask) on the GPU.

The reference's semantics hold for any solid set: solid cells keep w_i, the collision and the wall / inlet / outlet conditions skip
them, fluid cells pull w_i from them, and forces are the momentum exchange over solid->fluid links. The oracle runs on a mask too
(Oracle.solid is a writable view of the array its collision, BCs, initialisation and stability scan read), so it checks any geometry;
only its lbmo_forces recomputes the disc, so the forces here are recomputed in numpy with the reference's link rule."""
import numpy as np
import pytest

from tests.helpers import (ORACLE_PLANS, PLANS, TALL_F32, assert_forces_match, assert_group_is_whole, assert_matches_reference, disc,  # noqa: F401
                           host_staged_two_strips, lbm_gpu, masks, read_csv_rows, read_params, run_solver, square, strict, u_bar_rel, write_pgm)
from tests.reference import oracle_run

pytestmark = pytest.mark.gpu


# ---- 1. the disc passed as a mask is the analytic disc, bit for bit, on every plan -------------------------------------------
@pytest.mark.parametrize("size", [(1024, 256), (2048, 512)])
@pytest.mark.parametrize("plan", list(PLANS))
def test_disc_as_mask_is_the_analytic_disc(lbm, plan, size):
    nx, ny = size
    steps, of = 23, 7
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.08)
    runs = []
    for masked in (False, True):
        solid = None
        if masked:
            with lbm.Context(nx, ny, **kw) as probe:
                solid = probe.solid()
        with lbm.Context(nx, ny, options=PLANS[plan], solid=solid, **kw) as ctx:
            n = ctx.initialise()
            ctx.step(steps, of)
            ctx.step(1, 0)
            runs.append((n, ctx.populations("f_current"), ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(),
                         ctx.first_unstable_step(), ctx.solid(), ctx.kernel_name()))
    a, b = runs
    assert a[0] == b[0] and a[5] == b[5] and np.array_equal(a[6], b[6])
    if (PLANS[plan] or {}).get("tune") == 0:   # (a measured plan may differ between two measurements; its results may not)
        assert a[7] == b[7]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for u, v in zip(a[3], b[3]):
        assert np.array_equal(u, v)
    assert a[4] == b[4] and len(a[4]) == 4


def test_disc_as_mask_first_unstable_step(lbm):
    nx, ny = 1024, 256
    kw = dict(tau=0.5005, inlet_velocity=0.3, cylinder_radius=0.1)
    with lbm.Context(nx, ny, **kw) as probe:
        solid = probe.solid()
    got = []
    for s in (None, solid):
        for plan in ("rowil-col5-nt", "fast-rowil-col6", "rowil-site-nt"):
            with lbm.Context(nx, ny, options=PLANS[plan], solid=s, **kw) as ctx:
                ctx.initialise()
                ctx.step(400, 0)
                got.append(ctx.first_unstable_step())
    assert got[0] >= 0 and got[:3] == got[3:], got


# ---- 2. other geometries against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(masks(200, 64)))
def test_masks_against_the_oracle(lbm, name):
    nx, ny, steps, of = 200, 64, 60, 20        # (200 % 64 != 0: a ragged last tile column)
    kw = dict(inlet_velocity=0.05)
    mask = masks(nx, ny)[name]
    ref = oracle_run(nx, ny, steps, of, mask=mask, **kw)
    assert ref.solid_count == int(mask.sum())
    fast = {}
    for plan in ORACLE_PLANS:
        with lbm.Context(nx, ny, options=PLANS[plan], solid=mask, **kw) as ctx:
            assert ctx.initialise() == ref.solid_count
            assert np.array_equal(ctx.solid(), mask)
            ctx.step(steps, of)
            assert ctx.first_unstable_step() == ref.first_unstable
            if ref.first_unstable >= 0:
                continue
            log = ctx.drain_force_log()
            fn = ctx.populations("f_next")
            macros = ctx.macros()
        key = "strict" if strict(plan) else "fast"
        fast.setdefault(key, fn)
        assert np.array_equal(fn, fast[key]), plan      # every plan of one arithmetic mode: the same bits
        assert_matches_reference(plan, fn, macros, log, ref, u_bar_rel(ref), fast_rho=False)


def test_whole_domain_mask_forces_in_fixed_chunks(lbm):
    """A mask spread over the whole domain: the force box (here 640 x 224 cells) is cut into fixed chunks, one block each, summed in
    chunk order — the same bits on every plan and every repetition, and the reference's link rule."""
    nx, ny, steps, of = 640, 224, 21, 10
    kw = dict(inlet_velocity=0.04)
    mask = (np.random.default_rng(99).random((ny, nx)) < 0.02).astype(np.uint8)
    mask[0, 0] = mask[ny - 1, nx - 1] = 1
    ref = oracle_run(nx, ny, steps, of, mask=mask, **kw)
    assert ref.first_unstable == -1
    logs = []
    for plan in ("rowil-site-nt", "rowil-col5-nt", "rowil-col5-nt", "planar-fuse3-8"):
        with lbm.Context(nx, ny, options=PLANS[plan], solid=mask, **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            logs.append(ctx.drain_force_log())
    assert all(l == logs[0] for l in logs)
    assert_forces_match(logs[0], ref.forces, "every plan")


# ---- 3. strips --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["rowil-site-nt", "rowil-fuse3-12-nt-xcd", "rowil-col5-nt", "fast-rowil-col6"])
def test_group_strips_with_a_straddling_obstacle(lbm, plan):
    nx, ny, steps, of = 320, 100, 131, 45
    kw = dict(inlet_velocity=0.06)
    mask = square(nx, ny)
    mask[30:45, 150:170] = 1                  # straddles the face between the strips at row 37
    mask = disc(mask, 230, 59, 7)             # ... and the one at row 59
    with lbm.Context(nx, ny, options=PLANS[plan], solid=mask, **kw) as whole:
        solid = whole.initialise()
        whole.step(steps, of)
        w = (whole.macros(), whole.populations("f_next"), whole.drain_force_log())
    with lbm.Group(nx, ny, [(0, 37), (37, 22), (59, 41)], options=PLANS[plan], solid=mask, **kw) as g:
        assert g.initialise() == solid == int(mask.sum())
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert_group_is_whole(g, w)


@pytest.mark.parametrize("plan", [None, "rowil-col5-nt"])
def test_host_staged_strips_with_a_straddling_obstacle(lbm, plan):
    nx, ny = 1024, 256
    kw = dict(inlet_velocity=0.05)
    mask = disc(np.zeros((ny, nx), np.uint8), 200, 128, 20)
    mask[100:140, 500:520] = 1
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], solid=mask, **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    parts, solids = host_staged_two_strips(lbm, nx, ny, 12, 4, PLANS[plan] if plan else None, solid=mask, **kw)
    assert np.array_equal(solids[0], mask[:128]) and np.array_equal(solids[1], mask[128:])
    assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


# ---- 4. fp32 ----------------------------------------------------------------------------------------------------------------
def test_fp32_masked_run_against_fp64(lbm):
    nx, ny, steps = 1024, 256, 300
    kw = dict(inlet_velocity=0.05)
    mask = square(nx, ny)
    mask = disc(mask, 600, 100, 12)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], solid=mask, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        ref = ctx.macros()
    uscale = float(np.max(np.sqrt(ref[1] ** 2 + ref[2] ** 2)))
    out = {}
    for name, opts in (("auto", None), ("col5", PLANS["rowil-col5-nt"]), ("tall", TALL_F32)):
        with lbm.Context(nx, ny, precision="f32", options=opts, solid=mask, **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, 0)
            assert ctx.first_unstable_step() == -1
            if name == "tall":
                assert "k_stepc_col<float,6,8,7" in ctx.kernel_name().replace(" ", "")
            out[name] = ctx.macros()
    for name, m in out.items():
        er = float(np.max(np.abs(m[0] - ref[0])) / np.max(np.abs(ref[0])))
        eu = max(float(np.max(np.abs(m[1] - ref[1]))), float(np.max(np.abs(m[2] - ref[2])))) / uscale
        assert er < 2e-4 and eu < 2e-4, (name, er, eu)
        for a, b in zip(out["auto"], m):
            assert np.array_equal(a, b), name


# ---- 5. checkpoints ----------------------------------------------------------------------------------------------------------
def test_masked_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.07)
    mask = square(nx, ny)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], solid=mask, **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "m.ckpt")
        a.step(100, 50)
        ref = (a.populations("f_next"), a.drain_force_log())
    with lbm.Context(nx, ny, options=PLANS["rowil-col5-nt"], solid=mask, **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "m.ckpt")
        b.step(100, 50)
        assert np.array_equal(b.populations("f_next"), ref[0]) and b.drain_force_log() == ref[1]
    other = mask.copy()
    other[5, 5] = 1
    with lbm.Context(nx, ny, solid=other, **kw) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="different obstacle mask"):
            c.load_state(tmp_path / "m.ckpt")
    with lbm.Context(nx, ny, **kw) as d:           # unmasked: refuses the masked file; its own files keep the old layout
        d.initialise()
        with pytest.raises(lbm.LbmError, match="with an obstacle mask"):
            d.load_state(tmp_path / "m.ckpt")
        d.step(3, 0)
        d.save_state(tmp_path / "plain.ckpt")
        assert open(tmp_path / "plain.ckpt", "rb").read(8) == b"LBMCKPT1"
        d.load_state(tmp_path / "plain.ckpt")
    with lbm.Context(nx, ny, solid=mask, **kw) as e:
        e.initialise()
        with pytest.raises(lbm.LbmError, match="without an obstacle mask"):
            e.load_state(tmp_path / "plain.ckpt")


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------
def test_set_solid_mask_arguments(lbm):
    import ctypes as C
    nx, ny = 128, 32
    mask = square(nx, ny)
    with lbm.Context(nx, ny) as ctx:
        L, ub = ctx.L, C.POINTER(C.c_ubyte)
        ptr = mask.ctypes.data_as(ub)
        assert L.lbm_set_solid_mask(ctx.h, ptr, nx + 1, ny) == -1 and b"mask is" in L.lbm_last_error()
        assert L.lbm_set_solid_mask(ctx.h, ptr, nx, ny - 1) == -1
        assert L.lbm_set_solid_mask(ctx.h, None, nx, ny) == -1 and b"null" in L.lbm_last_error()
        assert L.lbm_set_solid_mask(ctx.h, ptr, nx, ny) == 0
        assert ctx.initialise() == int(mask.sum())
        assert L.lbm_set_solid_mask(ctx.h, ptr, nx, ny) == -1 and b"before lbm_initialise" in L.lbm_last_error()
        with pytest.raises(ValueError):
            lbm.Context(nx, ny, solid=mask[:, :-1])


# ---- 7. the host CLI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--gpus", "2", "--strips", "2"]])
def test_lbm_solver_obstacle_mask_matches_the_binding(lbm, tmp_path, extra):
    nx, ny, steps, of = 128, 48, 301, 100
    mask = np.zeros((ny, nx), np.uint8)
    mask[18:30, 30:42] = 1                    # square, frontal height D = 12
    write_pgm(tmp_path / "sq.pgm", mask * 255)
    u = 0.04
    args = ["--nx", str(nx), "--ny", str(ny), "--steps", str(steps), "--output-frequency", str(of), "--inlet-velocity", str(u),
            "--no-vtk", "--obstacle-mask", str(tmp_path / "sq.pgm")] + extra
    pr = run_solver(args, tmp_path)
    assert "frontal height D=12" in pr.stdout and f"Solid cells: {int(mask.sum())}" in pr.stdout
    rows = read_csv_rows(tmp_path / "forces.csv")
    with lbm.Context(nx, ny, inlet_velocity=u, solid=mask) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        log = ctx.drain_force_log()
    q = 0.5 * u * u * 12
    assert [int(r[0]) for r in rows] == [t for t, _, _ in log]
    for r, (t, fx, fy) in zip(rows, log):
        for got, want in zip(map(float, r[1:]), (fx, fy, fx / q, fy / q)):
            assert abs(got - want) <= 1.5e-8, (t, r)
    params = read_params(tmp_path / "simulation_params.csv")
    assert params["reference_length"] == "12" and params["obstacle_mask"].endswith("sq.pgm")
    assert abs(float(params["reynolds_number"]) - u * 12 / ((0.6 - 0.5) / 3.0)) < 1e-8
    # --reynolds sets the inlet velocity from D
    pr = run_solver(args[:4] + ["--steps", "2", "--output-frequency", "1", "--no-vtk", "--no-final", "--reynolds", "20",
                                "--obstacle-mask", str(tmp_path / "sq.pgm")] + extra, tmp_path)
    assert f"Inlet velocity = {20 * ((0.6 - 0.5) / 3.0) / 12:g}" in pr.stdout and "Reynolds number = 20" in pr.stdout, pr.stdout
