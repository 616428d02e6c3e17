"""GPU parity tests proper: the HIP path, called through the C-ABI (include/lbm_hip.h via ctypes), against
(1) the committed golden fixtures produced by the unmodified reference and (2) the CPU oracle on the same
inputs. The inputs of this path are analytic (no RNG: Grid::initialise is deterministic), so "seeded inputs"
means "same SimulationParams".

Tolerance (north_star): rho and u within 1e-10 relative (L-inf / L-inf; velocity components relative to
max|u|), Fx/Fy within 1e-10 relative. Observed on MI355X: see DESIGN.md §parity.
"""
import os

import numpy as np
import pytest

from tests.helpers import (FAST, PKG, PLANS, ROOT, TALL_F32, golden_params, lbm_gpu, linf_rel, load_golden, macro_errors, record,  # noqa: F401
                           strict)

pytestmark = pytest.mark.gpu
TOL = 1e-10


def fused_depth(plan_opts, steps_left, done, of):
    """The depth the library picks for the next launch (lbm_hip.hip: advance) when it is asked for exactly that many
    iterations with trailing_pair=1 — the host-staged strip drivers below must issue ONE launch per lbm_step call."""
    maxd = (plan_opts or {}).get("fuse", 2 if (plan_opts or {}).get("pair") else 1)
    deep = (plan_opts or {}).get("deep", 0)
    if deep:
        maxd = 3                                     # what is left of a segment goes to the three-/two-iteration kernels
        depths = {1: (6,), 6: (6, 5), 7: (6, 5)}.get(deep, ())      # a strip's ghost rows go six deep: no 7 / 8
        for d in depths:
            if steps_left >= d + 1 and all(of <= 0 or (done + j) % of != 0 for j in range(1, d)):
                return d
    for d in (3, 2):
        if d <= maxd and steps_left >= d + 1 and all(of <= 0 or (done + j) % of != 0 for j in range(1, d)):
            return d
    return 1


def run_gpu(lbm, g, plan=None, **extra):
    kw = golden_params(g)
    kw.update(extra)
    ctx = lbm.Context(options=PLANS[plan] if plan else None, **kw)
    ctx.initialise()
    ctx.step(int(g["p_steps"]), int(g["p_output_frequency"]))
    return ctx


def check_forces(rows, ref):
    """rows: [(t, fx, fy)] from the device log; ref: forces.csv rows of the reference (8 decimals)."""
    assert len(rows) == ref.shape[0]
    for (t, fx, fy), r in zip(rows, ref):
        assert t == int(r[0])
        assert abs(fx - r[1]) <= 0.5e-8 + 1e-12 and abs(fy - r[2]) <= 0.5e-8 + 1e-12


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", ["g1_128x32_s1", "g1_128x32_s2", "g1_128x32_s10", "g1_128x32_s100",
                                  "g2_256x64_s1", "g2_256x64_s100", "g2_256x64_s1000",
                                  "g6_inlet_cyl_64x32_s50", "g7_wall_cyl_64x32_s50"])
def test_golden_macros_forces_populations(lbm, name, plan):
    g = load_golden(name)
    with run_gpu(lbm, g, plan) as ctx:
        assert ctx.first_unstable_step() == -1
        assert np.array_equal(ctx.solid(), g["solid"]) and ctx.solid_count == int(g["solid"].sum())
        rho, ux, uy = ctx.macros()
        er, eu = macro_errors(rho, ux, uy, g["rho"], g["ux"], g["uy"])
        assert er < TOL and eu < TOL, (er, eu)
        assert abs(np.sqrt(ctx.max_velocity_sq()) - float(g["max_velocity"][0])) < TOL
        check_forces(ctx.drain_force_log(), g["forces"])
        if "f_current" in g:
            fc, fn = ctx.populations("f_current"), ctx.populations("f_next")
            assert linf_rel(fn, g["f_next"]) < TOL
            assert linf_rel(fc, g["f_current"]) < TOL
            ny, nx = int(g["p_ny"]), int(g["p_nx"])
            # N1/N2 ghost semantics are exact
            assert np.all(fn[1:ny + 1, 0, :] == 0.0) and np.all(fn[1:ny + 1, nx + 1, :] == 0.0)
            # (the reference evaluates the initial equilibrium with -ffast-math AVX2: equal to an ulp, not bitwise)
            for a, b in ((fn[0], g["f_next"][0]), (fn[ny + 1], g["f_next"][ny + 1]),
                         (fc[0], g["f_current"][0]), (fc[:, 0], g["f_current"][:, 0])):
                assert np.max(np.abs(a - b)) < 1e-15


@pytest.mark.parametrize("plan", list(PLANS))
def test_golden_re100_1024x256_s3000(lbm, plan):
    """BASELINE.json configs[1]: cylinder Re=100, 1024x256 fp64, 3000 steps."""
    g = load_golden("g4_1024x256_re100_s3000")
    with run_gpu(lbm, g, plan) as ctx:
        assert ctx.first_unstable_step() == -1 and ctx.solid_count == 441
        rho, ux, uy = ctx.macros()
        rows = [0, 1, 127, 128, 254, 255]
        for sel, tag in ((np.s_[::4, ::4], "_ds4"), (np.s_[rows, :], "_rows")):
            er, eu = macro_errors(rho[sel], ux[sel], uy[sel], g["rho" + tag], g["ux" + tag], g["uy" + tag])
            assert er < TOL and eu < TOL, (tag, er, eu)
        check_forces(ctx.drain_force_log(), g["forces"])


def test_golden_poiseuille(lbm):
    """BASELINE.json configs[0] on the GPU path: 256x64, cylinder disabled, 20000 steps."""
    g = load_golden("g3_poiseuille_256x64")
    with run_gpu(lbm, g) as ctx:
        assert ctx.solid_count == 0 and ctx.first_unstable_step() == -1
        _, ux, _ = ctx.macros()
        assert linf_rel(ux[:, 128], g["ux_x128"]) < TOL and linf_rel(ux[:, 192], g["ux_x192"]) < TOL
        ny = int(g["p_ny"])
        y = np.arange(ny, dtype=np.float64)
        shape = y * (ny - 1 - y)
        for col in (128, 192):
            u = ux[:, col]
            para = shape * (u.sum() / shape.sum())
            assert np.sqrt(np.mean((u - para) ** 2)) / u.max() < 2e-3
            assert abs(u.max() / u.mean() - 1.5) < 0.04


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", ["g8a_unstable_128x32", "g8b_unstable_128x32"])
def test_golden_unstable_timestep(lbm, name, plan):
    g = load_golden(name)
    with run_gpu(lbm, g, plan) as ctx:
        assert ctx.first_unstable_step() == int(g["unstable_t"])


@pytest.mark.parametrize("nx,ny,steps,kw", [
    (100, 37, 300, dict(inlet_velocity=0.08)),                      # ragged: nx not a multiple of the block
    (513, 65, 200, dict(inlet_velocity=0.1, cylinder_radius=0.11)),
    (8, 5, 40, dict(cylinder_x=-1.0, cylinder_radius=0.0)),          # tiny, no cylinder
    (2, 2, 10, dict(cylinder_x=-1.0, cylinder_radius=0.0)),          # every cell is a corner
    (300, 3, 50, dict(cylinder_x=-1.0, cylinder_radius=0.0)),        # one interior row between the walls
    (1024, 256, 500, dict(inlet_velocity=0.13020833)),
    (2048, 512, 120, dict(inlet_velocity=0.1)),                      # large enough for the measured plan
    (128, 70, 333, dict(inlet_velocity=0.09, cylinder_radius=0.1)),  # nx % 64 == 0, ny not a multiple of the tile
    (64, 9, 45, dict(cylinder_x=-1.0, cylinder_radius=0.0)),          # a single tile column, partial second tile row
])
@pytest.mark.parametrize("plan", ["auto", "planar-site", "rowil-vec-nt-alt", "planar-pair8-nt", "rowil-pair12-alt",
                                  "planar-fuse3-8", "rowil-fuse3-12-nt-xcd", "rowil-col5-nt", "planar-col6-alt",
                                  "rowil-deep6-nt", "rowil-fuse4-nt-xcd", "planar-fuse4-alt"] + FAST)
def test_against_oracle(lbm, nx, ny, steps, kw, plan):
    from oracle.oracle import Oracle, make_params
    of = max(1, steps // 5)
    o = Oracle(make_params(nx, ny, **kw))
    ref_forces = []
    bad = o.run(steps, of, ref_forces)
    with lbm.Context(nx, ny, options=PLANS[plan], **kw) as ctx:
        assert ctx.initialise() == o.solid_count()
        ctx.step(steps, of)
        assert ctx.first_unstable_step() == bad == -1
        rho, ux, uy = ctx.macros()
        er, eu = macro_errors(rho, ux, uy, o.rho, o.ux, o.uy)
        assert er < TOL and eu < TOL, (er, eu)
        # the library is built with -ffp-contract=off and evaluates the oracle's operation sequence: in fp64 the
        # populations are not merely within 1e-10 but bit-identical to the strict-IEEE CPU oracle
        if strict(plan):
            assert np.array_equal(ctx.populations("f_next"), o.f_next)
            assert np.array_equal(ctx.populations("f_current"), o.f_current)
        else:
            assert linf_rel(ctx.populations("f_next"), o.f_next) < TOL
            assert linf_rel(ctx.populations("f_current"), o.f_current) < TOL
        assert abs(ctx.max_velocity_sq() - o.max_velocity() ** 2) < TOL
        fscale = max(abs(r[1]) for r in ref_forces)
        for (t, fx, fy), r in zip(ctx.drain_force_log(), ref_forces):
            assert t == r[0] and abs(fx - r[1]) <= TOL * fscale and abs(fy - r[2]) <= TOL * fscale
        fx, fy = ctx.forces()            # == record_forces(t = steps)
        o.collide()
        ofx, ofy = o.forces()
        assert abs(fx - ofx) <= TOL * fscale and abs(fy - ofy) <= TOL * fscale


def test_contracted_arithmetic_is_plan_independent(lbm):
    """Every kernel family evaluates the same contracted per-cell sequence: site / vector / LDS-tile / register-column
    launches and a strip decomposition give identical bits (so the result does not depend on the launch schedule)."""
    nx, ny, steps, of = 320, 90, 240, 60
    kw = dict(inlet_velocity=0.07, cylinder_radius=0.1)
    out = []
    for plan in ("fast-site", "fast-vec-alt", "fast-rowil-col6", "fast-planar-col5", "fast-rowil-fuse3-12-xcd", "fast-planar-pair8",
                 "fast-rowil-fuse4-xcd", "fast-rowil-deep7", "fast-planar-deep8"):
        with lbm.Context(nx, ny, options=PLANS[plan], **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, of)
            out.append((ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log()))
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][2] == other[2]
        for u, v in zip(out[0][1], other[1]):
            assert np.array_equal(u, v)
    # ... and calls whose length makes the register family use all of its depths (20 = 7+7+6, 17 = 6+6+5, 5, 38 = 6x4+7+7)
    with lbm.Context(nx, ny, options=dict(PLANS["fast-rowil-col6"], trailing_pair=1), **kw) as ctx:
        ctx.initialise()
        for n in (20, 17, 5, 38, 60, 60, 39):
            ctx.step(n, of)
        ctx.step(1, of)
        assert ctx.steps_done == steps and np.array_equal(ctx.populations("f_next"), out[0][0]) and ctx.drain_force_log() == out[0][2]
    ctxs, _ = _run_strips(lbm, nx, ny, [(0, 40), (40, 13), (53, 37)], steps, of, pairs=True,
                          plans=["fast-rowil-fuse3-12-xcd", "fast-planar-pair8", "fast-rowil-col6"], **kw)
    assert np.array_equal(np.concatenate([c.populations("f_next")[1:-1] for c in ctxs], axis=0), out[0][0][1:-1])
    for c in ctxs:
        c.close()


def test_initial_state_accessors(lbm):
    """Right after initialise(): what Grid::initialise leaves (LBMGrid.h:185-246)."""
    from oracle.oracle import Oracle, make_params
    o = Oracle(make_params(64, 32, cylinder_radius=0.1))
    with lbm.Context(64, 32, cylinder_radius=0.1) as ctx:
        ctx.initialise()
        rho, ux, uy = ctx.macros()
        assert np.array_equal(rho, o.rho) and np.array_equal(ux, o.ux) and np.array_equal(uy, o.uy)
        assert np.array_equal(ctx.populations("f_current"), o.f_current)
        assert np.array_equal(ctx.populations("f_next"), o.f_next)


def _run_strips(lbm, nx, ny, bounds, steps, of, precision="f64", plans=None, pairs=False, **kw):
    """Strips on one GPU, host-staged halo exchange (lbm_halo_export/import) after every launch. pairs: launches
    fuse two iterations (trailing_pair) wherever the force cadence allows; the last launch is a single iteration."""
    plans = plans or [None] * len(bounds)

    def opts(pl):
        o = dict(PLANS[pl]) if pl else {}
        if pairs:
            o.update(trailing_pair=1)
        return o or None
    ctxs = [lbm.Context(nx, ny, y_start=y0, local_ny=n, precision=precision, options=opts(pl), **kw)
            for (y0, n), pl in zip(bounds, plans)]
    solid = sum(c.initialise() for c in ctxs)

    def exchange():
        ex = [c.halo_export(south=(k > 0), north=(k < len(ctxs) - 1)) for k, c in enumerate(ctxs)]
        for k, c in enumerate(ctxs):
            c.halo_import(south=ex[k - 1][1] if k > 0 else None,
                          north=ex[k + 1][0] if k < len(ctxs) - 1 else None)
    exchange()                            # P_0 edge rows
    done = 0
    while done < steps:
        # all strips must take the same number of iterations per launch: the smallest depth any of them would pick
        n = min(fused_depth(PLANS[pl] if pl else None, steps - done, done, of) for pl in plans) if pairs else 1
        for c in ctxs:
            c.step(n, of)
        done += n
        exchange()
    return ctxs, solid


def test_strips_match_single_domain_bitwise(lbm):
    """the y-strip decomposition must be decomposition-invariant (== the 1-rank result)."""
    nx, ny, steps, of = 192, 48, 120, 40
    kw = dict(inlet_velocity=0.06, cylinder_radius=0.12)
    with lbm.Context(nx, ny, **kw) as whole:
        solid = whole.initialise()
        whole.step(steps, of)
        w_rho, w_ux, w_uy = whole.macros()
        w_fn, w_fc = whole.populations("f_next"), whole.populations("f_current")
        w_log = whole.drain_force_log()
    # neighbouring strips may run different layouts: the halo rows are layout-independent
    ctxs, s_solid = _run_strips(lbm, nx, ny, [(0, 20), (20, 9), (29, 19)], steps, of,
                                plans=["planar-vec-alt", "rowil-site-nt", "rowil-vec-nt-alt"], **kw)
    assert s_solid == solid
    parts = [c.macros() for c in ctxs]
    for j, w in enumerate((w_rho, w_ux, w_uy)):
        assert np.array_equal(np.concatenate([p[j] for p in parts], axis=0), w)
    assert np.array_equal(np.concatenate([c.populations("f_next")[1:-1] for c in ctxs], axis=0), w_fn[1:-1])
    assert np.array_equal(np.concatenate([c.populations("f_current")[1:-1] for c in ctxs], axis=0), w_fc[1:-1])
    logs = [c.drain_force_log() for c in ctxs]
    for k, (t, fx, fy) in enumerate(w_log):
        assert all(l[k][0] == t for l in logs)
        assert abs(sum(l[k][1] for l in logs) - fx) <= 1e-13 * max(1.0, abs(fx))
        assert abs(sum(l[k][2] for l in logs) - fy) <= 1e-13
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("strip_plans", [["planar-pair8-nt", "rowil-pair12-alt", "rowil-pair12-alt"],
                                         ["planar-fuse3-8", "rowil-fuse3-12-nt-xcd", "rowil-fuse3-12-nt-xcd"],
                                         ["planar-col6-alt", "rowil-col5-nt", "rowil-fuse3-12-nt-xcd"],
                                         ["rowil-deep6-nt", "rowil-col5-nt", "planar-pair8-nt"]])
def test_strips_with_fused_launches_match_single_domain_bitwise(lbm, strip_plans):
    """Strips whose launches fuse two / three iterations: the LBM_HALO_ROWS-deep halo makes the recomputed edge rows
    identical to the neighbour's own; result == the one-domain run, bit for bit."""
    nx, ny, steps, of = 192, 60, 121, 40
    kw = dict(inlet_velocity=0.06, cylinder_radius=0.12)
    with lbm.Context(nx, ny, options=PLANS["planar-site"], **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w = whole.macros()
        w_fn = whole.populations("f_next")
        w_log = whole.drain_force_log()
    ctxs, _ = _run_strips(lbm, nx, ny, [(0, 25), (25, 8), (33, 27)], steps, of, pairs=True,
                          plans=strip_plans, **kw)
    parts = [c.macros() for c in ctxs]
    for j in range(3):
        assert np.array_equal(np.concatenate([p[j] for p in parts], axis=0), w[j])
    assert np.array_equal(np.concatenate([c.populations("f_next")[1:-1] for c in ctxs], axis=0), w_fn[1:-1])
    logs = [c.drain_force_log() for c in ctxs]
    for k, (tt, fx, fy) in enumerate(w_log):
        assert abs(sum(l[k][1] for l in logs) - fx) <= 1e-13 * max(1.0, abs(fx))
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("pair", [1, 2, 3])
def test_overlap_choreography_with_loopback_halo(lbm, pair):
    """The strip step as it runs under RCCL — edge rows first, exchange on the side stream, interior rows overlapped,
    two events — with the test-only loopback transport (the strip is its own neighbour: device copies instead of
    ncclSend/ncclRecv). Overlapped and serialised schedules must agree bit for bit over many launches."""
    nx, ny, steps = 1024, 96, 301
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    out = []
    # deep_halo=0: one exchange after every launch; deep_halo=1: one per two launches (the first one extended)
    for overlap, deep in ((0, 0), (0, 1), (1, 1), (1, 0), (2, 1), (2, 0)):
        with lbm.Context(nx, ny, options=dict(tune=0, layout=1, nt=1, fuse=pair, pair_ty=12, xcd=1,
                                              loopback=1, overlap=overlap, deep_halo=deep), **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, 50)
            ctx.sync()
            out.append((ctx.populations("f_next"), ctx.drain_force_log(), ctx.first_unstable_step()))
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0])
        assert out[0][1] == other[1] and out[0][2] == other[2]


@pytest.mark.parametrize("overlap,deep", [(1, 1), (0, 1), (1, 0), (0, 0), (2, 1), (2, 0)])
@pytest.mark.parametrize("plan", ["rowil-fuse3-12-nt-xcd", "rowil-pair12-alt", "rowil-site-nt", "fast-rowil-fuse3-12-xcd",
                                  "rowil-deep6-nt", "rowil-col5-nt", "fast-rowil-col6"])
def test_group_of_strips_on_one_device_matches_single_domain_bitwise(lbm, plan, overlap, deep):
    """In-process strips (lbm_group_*, the transport `lbm_solver --gpus N` uses) with the production choreography: edge
    bands on the side stream, every strip PULLING its neighbours' edge rows with exactly the pointers / offsets / counts
    of the RCCL branch (FaceSpans: top_rows -> ghost_s, bot_rows -> ghost_n), interior rows overlapped, extended first
    launch of a pair. Three uneven strips share the one GPU of the box (the peer copy degenerates to a device copy) and
    must reproduce the one-domain run bit for bit, for every overlap / halo-depth schedule."""
    nx, ny, steps, of = 320, 100, 271, 45
    kw = dict(inlet_velocity=0.06, cylinder_radius=0.12)
    # one host thread per strip (default) or the calling thread issuing for all of them
    opts = dict(PLANS[plan], overlap=overlap, deep_halo=deep, group_threads=0 if (overlap + deep) % 2 else 1)
    with lbm.Context(nx, ny, options=PLANS[plan], **kw) as whole:
        solid = whole.initialise()
        whole.step(steps, of)
        w = (whole.macros(), whole.populations("f_next"), whole.populations("f_current"), whole.drain_force_log(),
             whole.forces(), whole.max_velocity_sq())
    with lbm.Group(nx, ny, [(0, 37), (37, 22), (59, 41)], options=opts, **kw) as g:
        assert g.initialise() == solid
        g.step(steps, of)
        assert g.first_unstable_step() == -1 and g.steps_done == steps
        for u, v in zip(g.macros(), w[0]):
            assert np.array_equal(u, v)
        assert np.array_equal(g.populations("f_next"), w[1])
        assert np.array_equal(g.populations("f_current")[1:-1], w[2][1:-1])
        log = g.drain_force_log()
        assert [r[0] for r in log] == [r[0] for r in w[3]]
        for (t, fx, fy), (_, wx, wy) in zip(log, w[3]):
            assert abs(fx - wx) <= 1e-13 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-13
        fx, fy = g.forces()
        assert abs(fx - w[4][0]) <= 1e-13 * max(1.0, abs(w[4][0])) and abs(fy - w[4][1]) <= 1e-13
        assert g.max_velocity_sq() == w[5]
        with pytest.raises(lbm.LbmError, match="member of a group"):
            g.ctxs[0].step(1, 0)


@pytest.mark.parametrize("plan", [None, "rowil-deep6-nt", "rowil-deep8-nt", "rowil-col5-nt", "planar-col6-alt"])
def test_host_staged_strips_calling_patterns(lbm, plan):
    """The MPI-hosted calling pattern of INTEGRATION.md §C: lbm_step(4) = a fused launch of three iterations + a single
    one, then the caller exchanges the edge rows — on contexts that measured their own plan (None: large enough to time the
    candidates, deep ones included) and on pinned deep plans (the eight-iteration shape must fall back: a strip's ghost
    frame is six rows deep); also one launch of six per call with trailing_pair. All reproduce the one-domain run."""
    nx, ny = 1024, 256
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(48, 0)
        w_fn = whole.populations("f_next")
    for per_call, extra in ((4, {}), (6, dict(trailing_pair=1))):
        opts = dict(PLANS[plan] if plan else {}, **extra) or None
        ctxs = [lbm.Context(nx, ny, y_start=y0, local_ny=128, options=opts, **kw) for y0 in (0, 128)]
        try:
            for c in ctxs:
                c.initialise()

            def exchange():
                lo, hi = ctxs[0].halo_export(south=False, north=True), ctxs[1].halo_export(south=True, north=False)
                ctxs[0].halo_import(south=None, north=hi[0])
                ctxs[1].halo_import(south=lo[1], north=None)
            exchange()
            calls = [4] * 12 if per_call == 4 else [6] * 7 + [1] * 6     # (a snapshot needs a call that ends on a single iteration)
            for n in calls:
                for c in ctxs:
                    c.step(n, 0)
                exchange()
            parts = [c.populations("f_next") for c in ctxs]
        finally:
            for c in ctxs:
                c.close()
        # (each strip's array carries its own ghost frame: compare the interior rows)
        assert np.array_equal(parts[0][1:129], w_fn[1:129]) and np.array_equal(parts[1][1:129], w_fn[129:257])


@pytest.mark.parametrize("precision,ny,expect", [("f64", 200, "6-step 64x16"), ("f32", 200, "6-step 64x16"),
                                                 ("f64", 600, "6-step 64x32 in registers"), ("f32", 600, "6-step 64x32 in registers")])
def test_tall_strips_take_the_deep_plan_by_rule(lbm, precision, ny, expect):
    """A measured (tune=1) group runs six iterations per launch with one exchange per launch where its strips have 64 rows or
    more — on 64x16 LDS tiles (the shortest launch: such strips are bound by the chain edge band -> exchange -> edge band), from
    192 rows on 64x32 regions held in registers (k_stepc_col: the highest throughput) — chosen by rule from the global grid and
    the strip count, so that every strip (every rank of a multi-process run) issues the same launch depths; and reproduces
    the one-domain run bit for bit (fp64 and fp32)."""
    nx, steps, of = 512, 333, 70
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1, precision=precision)
    ftol = 1e-13 if precision == "f64" else 1e-5        # partial force sums are added in a different order
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
    for extra in (dict(), dict(overlap=0), dict(group_threads=0)):
        with lbm.Group(nx, ny, 3, options=extra or None, **kw) as g:
            g.initialise()
            assert all(expect in m.plan() for m in g.ctxs), [m.plan() for m in g.ctxs]
            g.step(steps, of)
            assert g.first_unstable_step() == -1
            assert np.array_equal(g.populations("f_next"), w_fn)
            log = g.drain_force_log()
            assert [r[0] for r in log] == [r[0] for r in w_log]
            for (t, fx, fy), (_, wx, wy) in zip(log, w_log):
                assert abs(fx - wx) <= ftol * max(1.0, abs(wx)) and abs(fy - wy) <= ftol


@pytest.mark.parametrize("ny,bounds,expect", [(200, [(0, 150), (150, 14), (164, 36)], "6-step 64x16"),
                                              (600, [(0, 480), (480, 14), (494, 106)], "6-step 64x32 in registers")])
def test_strongly_uneven_strips_under_the_deep_rule(lbm, ny, bounds, expect):
    """The strip rule picks the six-iteration kernel from ny / strips alone, whatever the strips' real heights: a middle strip
    of 14 rows — shorter than one band of tiles, i.e. all edge — between tall ones must still reproduce the one-domain run bit
    for bit, with one host thread per strip and with the calling thread issuing for all."""
    nx, steps, of = 384, 187, 60
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
    for extra in (dict(), dict(group_threads=0, overlap=0)):
        with lbm.Group(nx, ny, bounds, options=extra or None, **kw) as g:
            g.initialise()
            assert all(expect in m.plan() for m in g.ctxs), [m.plan() for m in g.ctxs]
            g.step(steps, of)
            assert g.first_unstable_step() == -1
            assert np.array_equal(g.populations("f_next"), w_fn)
            assert [r[0] for r in g.drain_force_log()] == [r[0] for r in w_log]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("threads", [1, 0])
def test_a_failing_strip_is_an_error_not_a_hang(lbm, threads):
    """A group whose members disagree (one strip pinned to single-iteration launches) must come back from lbm_group_step
    with an error on every driver — with one host thread per strip the decision to abort is taken once per rendezvous, so no
    thread is left waiting at a barrier the others never reach — and the group stays usable for teardown."""
    nx, ny = 256, 120
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    opts = dict(PLANS["rowil-fuse3-12-nt-xcd"], group_threads=threads)
    with lbm.Group(nx, ny, 3, options=opts, **kw) as g:
        g.ctxs[1].set_option("fuse", 1)
        g.initialise()
        with pytest.raises(lbm.LbmError, match="disagree"):
            g.step(30, 0)
        with pytest.raises(lbm.LbmError):          # ... and again: the pool's threads are parked, not stuck
            g.step(30, 0)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("point", [0, 1, 2])
def test_a_strip_that_fails_between_two_rendezvous_is_an_error_not_a_hang(lbm, point):
    """a member whose runtime call fails BETWEEN two rendezvous of the group's threads (injected: strip 1, third
    launch, before the first / second / third rendezvous) must not skip an arrival — every error goes through report() and the
    whole group leaves at the next rendezvous. The call returns the strip's error, the pool's threads are parked again, and the
    group, re-initialised, reproduces the one-domain run bit for bit."""
    nx, ny, steps = 256, 120, 31
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as whole:
        whole.initialise()
        whole.step(steps, 0)
        w_fn = whole.populations("f_next")
    with lbm.Group(nx, ny, 3, options=PLANS["rowil-fuse3-12-nt-xcd"], **kw) as g:
        g.initialise()
        g.ctxs[1].set_option("debug_fault_point", point)
        g.ctxs[1].set_option("debug_fault_launch", 2)
        with pytest.raises(lbm.LbmError, match=f"injected fault: strip 1, launch 2, point {point}"):
            g.step(steps, 0)
        g.initialise()
        g.step(steps, 0)
        assert g.first_unstable_step() == -1 and np.array_equal(g.populations("f_next"), w_fn)


@pytest.mark.timeout(120)
def test_a_stalled_strip_turns_into_a_timeout_that_names_it(lbm):
    """Every host-side wait of a group is bounded (round 5; rounds 3-4 waited on a std::barrier and an untimed condition
    variable): a strip that does not reach a rendezvous within "wait_timeout_ms" (injected: strip 2 sleeps 1.5 s between the first
    and the second rendezvous of its second launch) makes lbm_group_step return LBM_ERR_TIMEOUT within the bound, naming the strip and
    where it was last seen; the group refuses further work and its teardown waits for the straggler instead of freeing under it."""
    import time
    nx, ny = 256, 120
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Group(nx, ny, 3, options=dict(PLANS["rowil-fuse3-12-nt-xcd"], wait_timeout_ms=250), **kw) as g:
        g.initialise()
        g.step(7, 0)                    # (warm: the kernels' code object is loaded before the clock starts)
        for c in g.ctxs:
            c.sync()
        for key, v in (("debug_fault_point", 1), ("debug_fault_stall_ms", 1500), ("debug_fault_launch", 1)):
            g.ctxs[2].set_option(key, v)
        t0 = time.time()
        with pytest.raises(lbm.LbmError, match=r"lbm_hip error -5: strip [01] waited 250 ms at rendezvous 2 of launch 1 of this call for: strip 2 \(last seen at rendezvous 1 of launch 1\)"):
            g.step(30, 0)
        assert time.time() - t0 < 1.4          # back before the straggler's 1.5 s are over
        with pytest.raises(lbm.LbmError, match="timed out earlier"):
            g.step(1, 0)


@pytest.mark.timeout(120)
def test_lbm_sync_is_bounded_on_request(lbm):
    """With "wait_timeout_ms" set, lbm_sync polls the streams instead of blocking in hipStreamSynchronize: with a bound far below the
    queued work (a few thousand iterations of the headline grid) it returns LBM_ERR_TIMEOUT naming the stream and the iteration the
    queue reaches; with the bound lifted the same call drains the queue through the blocking path (the default: polling a stream while a
    short timed window runs costs throughput, profiles/r04/README.md §3 — a watchdog thread names a blocking wait that stalls)."""
    with lbm.Context(4096, 1024, inlet_velocity=0.0651, options=dict(PLANS["fast-rowil-col6"], trailing_pair=1)) as c:
        c.initialise()
        c.sync()
        c.set_option("wait_timeout_ms", 2)
        c.step(3000, 0)
        with pytest.raises(lbm.LbmError, match=r"lbm_hip error -5: compute stream of the strip of rows 0..1024 on device 0 still busy after 2 ms \(work queued up to iteration 3000\)"):
            c.sync()
        c.set_option("wait_timeout_ms", 0)
        c.sync()
        assert c.steps_done == 3000 and c.first_unstable_step() == -1


@pytest.mark.timeout(180)
def test_a_blocking_wait_that_stalls_is_named_by_the_watchdog(tmp_path):
    """lbm_sync's default is the blocking hipStreamSynchronize; a wait that outlives the bound (LBM_WAIT_TIMEOUT_MS, here 300 ms against
    ~1.2 s of queued work) is not interrupted but NAMED: one STALL line on stderr and in the LBM_TRACE file, with the strip, the stream
    and the iteration — silence can no longer be the only record of a run that hangs in the runtime."""
    import subprocess
    import sys
    trace = tmp_path / "trace.txt"
    code = (f"import importlib, sys; sys.path.insert(0, {ROOT!r}); lbm = importlib.import_module({PKG!r})\n"
            "with lbm.Context(8192, 2048, inlet_velocity=0.0325, options=dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=1)) as c:\n"
            "    c.initialise(); c.sync(); c.step(3000, 0); c.sync(); assert c.first_unstable_step() == -1\n")      # (3000 launches of ~0.4 ms: any queue holds them, the wait is the sync)
    out = subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, LBM_TRACE=str(trace), LBM_WAIT_TIMEOUT_MS="300"), timeout=170,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert "lbm_hip: STALL: hipStreamSynchronize(compute stream) of the strip of rows 0..2048 on device 0, work queued up to iteration 3000" in out.stderr, out.stderr[-500:]
    assert any(" STALL " in ln for ln in trace.read_text().splitlines())


@pytest.mark.timeout(180)
def test_the_trace_file_names_the_last_thing_started(tmp_path):
    """LBM_TRACE=<file>: one flushed line per coarse event (initialise / step / destroy, begin and end), so that a run killed for
    being silent leaves its last started call on record (a seven-minute stall left an empty log)."""
    import subprocess
    import sys
    trace = tmp_path / "trace.txt"
    code = (f"import importlib, sys; sys.path.insert(0, {ROOT!r}); lbm = importlib.import_module({PKG!r})\n"
            "with lbm.Context(256, 64) as c:\n    c.initialise(); c.step(7, 0); c.sync()\n")
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, LBM_TRACE=str(trace)), timeout=170)
    lines = trace.read_text().splitlines()
    tags = [ln.split()[5] for ln in lines]
    assert tags[0] == "initialise" and "step" in tags and tags[-1] == "destroy" and lines[-1].endswith("end")
    assert any("t=0 +7 begin" in ln for ln in lines)


def test_group_checkpoint_restart(lbm, tmp_path):
    """Per-strip checkpoints of a group, restored into a fresh group (lbm_group_refresh_halos), continue bit-exactly."""
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.07, cylinder_radius=0.1)
    with lbm.Group(nx, ny, 3, options=PLANS["rowil-fuse3-12-nt-xcd"], **kw) as a:
        a.initialise()
        a.step(137, 0)
        for k, c in enumerate(a.ctxs):
            c.save_state(tmp_path / f"s{k}.ckpt")
        a.step(200, 50)
        ref = (a.macros(), a.populations("f_next"), a.drain_force_log())
    with lbm.Group(nx, ny, 3, options=PLANS["rowil-fuse3-12-nt-xcd"], **kw) as b:
        b.initialise()
        for k, c in enumerate(b.ctxs):
            c.load_state(tmp_path / f"s{k}.ckpt")
        b.refresh_halos()
        assert b.steps_done == 137
        b.step(200, 50)
        got = (b.macros(), b.populations("f_next"), b.drain_force_log())
    for u, v in zip(ref[0], got[0]):
        assert np.array_equal(u, v)
    assert np.array_equal(ref[1], got[1]) and ref[2] == got[2]


def test_checkpoint_restart_is_bit_exact(lbm, tmp_path):
    """Save at iteration 137, restore into a fresh context (different plan), continue: identical to the uninterrupted run."""
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.07, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=PLANS["planar-pair8-nt"], **kw) as a:
        a.initialise()
        a.step(137, 0)
        a.save_state(tmp_path / "s.ckpt")
        a.step(200, 50)
        ref = (a.macros(), a.populations("f_next"), a.drain_force_log())
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as b:
        b.initialise()
        b.load_state(tmp_path / "s.ckpt")
        assert b.steps_done == 137
        with pytest.raises(lbm.LbmError, match="snapshot unavailable"):
            b.macros()
        b.step(200, 50)
        got = (b.macros(), b.populations("f_next"), b.drain_force_log())
    for u, v in zip(ref[0], got[0]):
        assert np.array_equal(u, v)
    assert np.array_equal(ref[1], got[1]) and ref[2] == got[2]
    with lbm.Context(nx, ny, inlet_velocity=0.08, cylinder_radius=0.1) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="different parameters"):
            c.load_state(tmp_path / "s.ckpt")


@pytest.mark.parametrize("plan,steps,of,trailing,launches", [
    ("rowil-col5-nt", 20, 0, 1, 4),         # 5+5+5+5: four launches at the plan's own depth
    ("planar-col6-alt", 20, 0, 1, 3),       # 7+7+6 on the six-iteration plan (the bench's): a whole domain may fuse seven
    ("rowil-deep6-nt", 20, 0, 1, 4),        # 6+6+4+4 rather than 6+6+6+2
    ("rowil-deep8-nt", 19, 0, 1, 3),        # 8+8+3
    ("rowil-col5-nt", 20, 0, 0, 4),         # 7+7+5 and the single last iteration of a call that may be read back
    ("rowil-col5-nt", 24, 10, 1, 5),        # force outputs at 10 and 20 end the fused segments: 5+5 | 5+5 | 4
    ("rowil-fuse3-12-nt-xcd", 20, 0, 1, 6), # 4+4+3+3+3+3
    ("rowil-col5-nt", 22, 0, 1, 4),         # 6+6+5+5 / 7+5+5+5: the register family splits without a slow tail
    ("planar-col6-alt", 20, 0, 0, 4),       # 7+7+5 and the single last iteration
    ("planar-col6-alt", 38, 0, 1, 6),       # 6+6+6+6+7+7 rather than six sixes and a two
])
def test_a_call_is_split_into_full_rate_launches(lbm, plan, steps, of, trailing, launches):
    """plan_launch: the iterations of a call (between force outputs) are split into the cheapest sequence of the depths the
    plan has — no one- or two-iteration tail where a different split avoids it — and the result is that of single launches."""
    nx, ny = 256, 96
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as one:
        one.initialise()
        one.step(steps + 1, of)
        ref = one.populations("f_next")
    with lbm.Context(nx, ny, options=dict(PLANS[plan], trailing_pair=trailing, timing=1), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, of)
        _, n, its = ctx.last_step_stats()
        assert (n, its) == (launches, steps)
        ctx.step(1, of)                      # (a snapshot needs a call that ends on a single iteration)
        assert np.array_equal(ctx.populations("f_next"), ref)


def test_c4_grid_8192x2048_single_gpu(lbm):
    """BASELINE.json configs[3] grid (8192x2048, Re=200) on ONE GPU (the 8-GPU strip run belongs to the driver), over the
    300-iteration window SURVEY §8d C4 asks for (200-500): strict arithmetic on the measured plan — populations bit-identical
    to the oracle — and the bench's contracted arithmetic on its measured plan within the north-star 1e-10 on rho, u and the
    momentum-exchange forces; then decomposition invariance for 8 strips."""
    from oracle.oracle import Oracle, make_params
    nx, ny, steps = 8192, 2048, 300
    kw = dict(inlet_velocity=0.03255208)
    o = Oracle(make_params(nx, ny, **kw))
    assert o.run(steps) == -1 and o.solid_count() == 32681
    o_fn = o.f_next.copy()
    o_m = (o.rho.copy(), o.ux.copy(), o.uy.copy())      # (collide() below moves the oracle's macros on to the next iteration)
    o.collide()
    ofx, ofy = o.forces()
    with lbm.Context(nx, ny, **kw) as ctx:
        assert ctx.initialise() == 32681
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        assert np.array_equal(ctx.populations("f_next"), o_fn)
        w = ctx.macros()
        er, eu = macro_errors(*w, *o_m)
        strict_plan = ctx.plan()
    with lbm.Context(nx, ny, options=dict(arith=1), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        cr, cu = macro_errors(*ctx.macros(), *o_m)
        fx, fy = ctx.forces()
        cf = max(abs(fx - ofx), abs(fy - ofy)) / abs(ofx)
        record("c4_8192x2048_f64_300", strict_rho=er, strict_u=eu, contracted_rho=cr, contracted_u=cu, contracted_force=cf,
               strict_plan=strict_plan, contracted_plan=ctx.plan())
        print(f"C4 x {steps}: strict rho {er:.2e} u {eu:.2e} (populations bit-equal); contracted rho {cr:.2e} u {cu:.2e} F {cf:.2e} [{ctx.plan()}]")
        assert er < TOL and eu < TOL and cr < TOL and cu < TOL and cf < TOL, (er, eu, cr, cu, cf)
    o.close()
    del o_fn, o_m
    short = 12
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(short, 0)
        w = ctx.macros()
    ctxs, _ = _run_strips(lbm, nx, ny, lbm.partition_rows(ny, 8), short, 0, pairs=True,
                          plans=["rowil-fuse3-12-nt-xcd"] * 8, **kw)
    parts = [c.macros() for c in ctxs]
    for j in range(3):
        assert np.array_equal(np.concatenate([p[j] for p in parts], axis=0), w[j])
    for c in ctxs:
        c.close()


def test_rccl_calls_on_a_one_rank_communicator(lbm):
    """The production RCCL exchange (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on the side stream, same counts,
    datatype and pointers as between strips) exercised on ONE GPU: a one-rank communicator sending to itself
    (loopback=2). Must equal the device-copy loopback bit for bit, overlapped and serialised."""
    nx, ny, steps = 1024, 96, 151
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    out = []
    for loopback, overlap in ((1, 0), (2, 1), (2, 0), (2, 2)):
        with lbm.Context(nx, ny, options=dict(tune=0, layout=1, nt=1, fuse=3, pair_ty=12, xcd=1,
                                              loopback=loopback, overlap=overlap), **kw) as ctx:
            if loopback == 2:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            ctx.step(steps, 50)
            ctx.sync()
            out.append((ctx.populations("f_next"), ctx.drain_force_log(), ctx.first_unstable_step()))
            if loopback == 2:
                assert np.allclose(ctx.allreduce([1.5, -2.0], "sum"), [1.5, -2.0])      # ncclAllReduce path
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][1] == other[1] and out[0][2] == other[2]


@pytest.mark.parametrize("loopback", [1, 2])
@pytest.mark.parametrize("overlap", [1, 0])
def test_launch_groups_replayed_from_a_graph_match_the_eager_path(lbm, loopback, overlap):
    """A strip with a device transport on a deep plan replays four launch groups (edge bands, events, exchange, interior rows)
    per hipGraphLaunch instead of issuing them call by call. Same bits as the eager path — populations, force log across
    output iterations that cut the replays short, and the FIRST UNSTABLE ITERATION of a run that blows up inside a replayed
    stretch (the kernels' iteration numbers are relative to a device word the graph advances) — with device copies and with
    RCCL send/recv to self as the transport, overlapped and serialised."""
    nx, ny = 512, 160
    base = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, loopback=loopback, overlap=overlap)
    for kw, steps, of in ((dict(inlet_velocity=0.05, cylinder_radius=0.1), 437, 150),
                          (dict(inlet_velocity=0.05, cylinder_radius=0.1, tau=0.5006), 700, 0)):        # the second one blows up
        out = []
        for graph in (0, 1):
            with lbm.Context(nx, ny, options=dict(base, graph=graph), **kw) as ctx:
                if loopback == 2:
                    ctx.comm_init(0, 1, ctx.comm_unique_id())
                ctx.initialise()
                ctx.step(steps, of)
                ctx.step(1, of)
                ctx.sync()
                bad = ctx.first_unstable_step()
                out.append((bad, ctx.populations("f_next") if bad == -1 else None, ctx.drain_force_log() if bad == -1 else None,
                            ctx.graph_replays()))
        assert out[0][3] == 0 and out[1][3] >= 2, (out[0][3], out[1][3])
        assert out[0][0] == out[1][0]
        if "tau" in kw:
            assert out[0][0] > 48, out[0][0]          # (it did blow up, and after the first replays)
        else:
            assert out[0][0] == -1 and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_strip_schedule_is_measured_and_result_invariant(lbm):
    """With a communicator attached and nothing pinned, lbm_initialise times the four exchange schedules (overlapped /
    serialised x deep / shallow halo) with the real transport — here RCCL send/recv to self on a one-rank communicator —
    and keeps the fastest; whatever it picks, the result equals the pinned-schedule run bit for bit."""
    nx, ny, steps = 1024, 128, 151
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    out = []
    for opts in (dict(tune=0, layout=1, nt=1, fuse=3, pair_ty=12, xcd=1, loopback=2, overlap=0, deep_halo=0),
                 dict(loopback=2), dict(loopback=2, overlap=1), dict(loopback=2, arith=0, deep_halo=1)):
        with lbm.Context(nx, ny, options=opts, **kw) as ctx:
            ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            sched = ctx.strip_schedule()
            if "tune" in opts:
                assert "fixed by options" in sched
            else:
                assert "measured" in sched, sched
                assert "row-interleaved" in ctx.plan()
            ctx.step(steps, 50)
            ctx.sync()
            # (interior rows: in the self-neighbour test set-up the corner ghosts of the ghost rows, which no result depends
            # on, hold 0 after an exchange and the initial equilibrium after an extended launch)
            out.append((ctx.populations("f_next")[1:-1], ctx.drain_force_log(), ctx.first_unstable_step()))
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][1] == other[1] and out[0][2] == other[2]


def test_strips_two_launches_per_exchange_match_single_domain_bitwise(lbm):
    """Host-staged strips exchanging their LBM_HALO_ROWS edge rows once per TWO launches (6 iterations): the first
    launch of each call also recomputes three ghost rows per internal face. == the one-domain run, bit for bit."""
    nx, ny, of = 192, 90, 12
    calls = 14
    steps = 6 * calls + 1
    kw = dict(inlet_velocity=0.06, cylinder_radius=0.12)
    with lbm.Context(nx, ny, options=PLANS["planar-site"], **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w = whole.macros()
        w_fn = whole.populations("f_next")
        w_log = whole.drain_force_log()
    bounds = [(0, 31), (31, 14), (45, 45)]
    plans = ["planar-fuse3-8", "rowil-fuse3-12-nt-xcd", "rowil-fuse3-12-nt-xcd"]
    ctxs = [lbm.Context(nx, ny, y_start=y0, local_ny=n, options=dict(PLANS[pl], trailing_pair=1), **kw)
            for (y0, n), pl in zip(bounds, plans)]
    for c in ctxs:
        c.initialise()

    def exchange():
        ex = [c.halo_export(south=(k > 0), north=(k < len(ctxs) - 1)) for k, c in enumerate(ctxs)]
        for k, c in enumerate(ctxs):
            c.halo_import(south=ex[k - 1][1] if k > 0 else None, north=ex[k + 1][0] if k < len(ctxs) - 1 else None)
    exchange()
    for _ in range(calls):
        for c in ctxs:
            c.step(6, of)           # [3 iterations, extended][3 iterations] — of = 12 falls on call boundaries
        exchange()
    for c in ctxs:
        c.step(1, of)
    exchange()
    parts = [c.macros() for c in ctxs]
    for j in range(3):
        assert np.array_equal(np.concatenate([p[j] for p in parts], axis=0), w[j])
    assert np.array_equal(np.concatenate([c.populations("f_next")[1:-1] for c in ctxs], axis=0), w_fn[1:-1])
    logs = [c.drain_force_log() for c in ctxs]
    assert [r[0] for r in logs[0]] == [r[0] for r in w_log]
    for k, (tt, fx, fy) in enumerate(w_log):
        assert abs(sum(l[k][1] for l in logs) - fx) <= 1e-13 * max(1.0, abs(fx))
    with pytest.raises(lbm.LbmError, match="at most two launches"):
        ctxs[1].step(9, 0)          # a third launch would need fresh ghost rows
    for c in ctxs:
        c.close()


def test_reinitialise_and_destroy_release_device_memory(lbm):
    """A second lbm_initialise (new plan measurement, new buffers) must not keep the first one's population buffers, an
    error path of the plan search must not either, and lbm_destroy returns everything (hipMemGetInfo)."""
    nx, ny = 2048, 512
    with lbm.Context(64, 32) as warm:      # the runtime's one-time allocations (code objects, queues: ~170 MB) happen here
        warm.initialise()
    # ... and the queue's scratch memory (~29 MB, kept by the runtime): the strict register kernel spills 12 VGPRs
    with lbm.Context(256, 64, options=dict(tune=0, layout=1, nt=1, xcd=1, deep=7)) as warm:
        warm.initialise()
        warm.step(12, 0)
    free0, _ = lbm.device_memory(0)
    with lbm.Context(nx, ny, inlet_velocity=0.05) as ctx:
        ctx.initialise()
        ctx.step(10, 0)
        ctx.macros()
        ctx.sync()
        free1, _ = lbm.device_memory(0)
        for _ in range(3):
            ctx.initialise()
            ctx.step(10, 0)
            ctx.macros()
        ctx.sync()
        free2, _ = lbm.device_memory(0)
        assert abs(free1 - free2) <= 8 << 20, (free1, free2)      # (allocation granularity of differently laid-out plans)
        used = free0 - free2
        assert used < 3 * 2 * 9 * (nx + 32) * (ny + 12) * 8, used   # two buffers (+ scratch, macros), not 2 x (initialisations)
    free3, _ = lbm.device_memory(0)
    assert abs(free3 - free0) <= 8 << 20, (free0, free3)


def test_graphs_and_group_threads_are_released(lbm):
    """Contexts that captured a launch-group graph (re-initialised in between: the graph holds buffer addresses) and groups with
    their parked host threads come and go without leaving device memory or threads behind (the runtime's own one-time
    allocations — graph pools, scratch, per-thread state — are taken by two warm-up rounds: measured, they stop growing there)."""
    def threads():
        return int(next(l for l in open("/proc/self/status") if l.startswith("Threads:")).split()[1])
    base = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7)

    def round_(k):
        with lbm.Context(512, 160, inlet_velocity=0.05, options=dict(base, loopback=1, overlap=k % 2)) as ctx:
            ctx.initialise()
            ctx.step(120, 0)
            assert ctx.graph_replays() >= 2
            ctx.initialise()                       # drops the graph with the buffers it was captured on
            ctx.step(120, 0)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
        t_before = threads()
        with lbm.Group(256, 120, 3, options=dict(base, deep=1, group_threads=1)) as g:
            g.initialise()
            g.step(60, 0)
            assert threads() >= t_before + 2       # one parked thread per strip beyond the first
    for k in range(2):
        round_(k)
    free0, _ = lbm.device_memory(0)
    t0 = threads()
    for k in range(6):
        round_(k)
    free1, _ = lbm.device_memory(0)
    assert abs(free1 - free0) <= 8 << 20, (free0, free1)
    assert threads() <= t0, (t0, threads())


def test_snapshot_refused_after_trailing_pair(lbm):
    with lbm.Context(128, 32, options=dict(tune=0, fuse=3, trailing_pair=1)) as ctx:
        ctx.initialise()
        ctx.step(3, 0)
        with pytest.raises(lbm.LbmError, match="snapshot unavailable"):
            ctx.macros()
        ctx.step(1, 0)
        ctx.macros()


def test_fp32_variant_tracks_fp64(lbm):
    """BASELINE.json configs[4] is an fp32 variant the reference does not have: parity is against the fp64 result
    at an fp32-appropriate tolerance (stated: 2e-4 relative on rho and u after 1000 steps at 256x64)."""
    nx, ny, steps = 256, 64, 1000
    kw = dict(inlet_velocity=0.05)
    out = {}
    for prec, plan in (("f64", None), ("f32", None), ("f32b", "rowil-vec-nt-alt"), ("f32c", "planar-site"),
                       ("f32d", "planar-pair8-nt"), ("f32e", "rowil-fuse3-12-nt-xcd")):
        with lbm.Context(nx, ny, precision=prec[:3], options=PLANS[plan] if plan else None, **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, 0)
            assert ctx.first_unstable_step() == -1
            out[prec] = ctx.macros()
    er, eu = macro_errors(*out["f32"], *out["f64"])
    assert er < 2e-4 and eu < 2e-4, (er, eu)
    for other in ("f32b", "f32c", "f32d", "f32e"):       # every fp32 formulation is the same arithmetic: bit-identical
        for a, b in zip(out["f32"], out[other]):
            assert np.array_equal(a, b)


def test_fp32_tracks_the_oracle_on_fused_plans_1024x256(lbm):
    """fp32 parity where the fused kernels and the measured plan are in play: BASELINE.json configs[1] grid (1024x256,
    Re=100), 1000 iterations, against the fp64 ORACLE (the reference has no fp32 path; the oracle is pinned to the reference).
    Stated tolerance: 1e-3 relative on rho and on u (L-inf / L-inf, u relative to max|u|) — fp32 carries 6e-8 per operation
    and 1000 iterations of a chaotic wake amplify it; measured on MI355X: DESIGN.md §4 / profiles/r03/parity_measured.jsonl.
    Every fp32 plan must agree with every other bit for bit, and this library's fp64 path must sit on the oracle."""
    from oracle.oracle import Oracle, make_params
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.13020833)
    o = Oracle(make_params(nx, ny, **kw))
    assert o.run(steps) == -1
    ref = (o.rho.copy(), o.ux.copy(), o.uy.copy())
    o.close()
    with lbm.Context(nx, ny, precision="f64", **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        er, eu = macro_errors(*ctx.macros(), *ref)
        assert er < TOL and eu < TOL, (er, eu)
    out = {}
    for plan in ("auto", "rowil-fuse3-12-nt-xcd", "rowil-fuse4-nt-xcd", "rowil-deep6-nt", "rowil-pair12-alt", "planar-site",
                 "rowil-col5-nt", "planar-col6-alt"):
        with lbm.Context(nx, ny, precision="f32", options=PLANS[plan], **kw) as ctx:
            ctx.initialise()
            ctx.step(steps, 0)
            assert ctx.first_unstable_step() == -1
            out[plan] = ctx.macros()
    with lbm.Context(nx, ny, precision="f32", options=TALL_F32, **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1 and "k_stepc_col<float,6,8,7" in ctx.kernel_name().replace(" ", "")
        out["rowil-col7-tall"] = ctx.macros()
    er, eu = macro_errors(*out["auto"], *ref)
    print(f"fp32 vs the fp64 oracle, 1024x256 x {steps}: rho {er:.3e}, u {eu:.3e}")
    # stated tolerance 2e-4 = about twice what was measured on MI355X (rho 1.2e-5, u 9.2e-5; SURVEY §8d C5: "≈1e-4 rel on u after
    # 1000 steps; state the tolerance measured") — round 3 asserted 1e-3, ten times the measurement
    assert er < 2e-4 and eu < 2e-4, (er, eu)
    for plan, m in out.items():
        for a, b in zip(out["auto"], m):
            assert np.array_equal(a, b), plan
    with lbm.Context(nx, ny, precision="f32", options=PLANS["fast-auto"], **kw) as ctx:      # contracted fp32
        ctx.initialise()
        ctx.step(steps, 0)
        cr, cu = macro_errors(*ctx.macros(), *ref)
        print(f"fp32 contracted vs the fp64 oracle: rho {cr:.3e}, u {cu:.3e}")
        assert cr < 2e-4 and cu < 2e-4, (cr, cu)
    record("c2_1024x256_f32_vs_oracle_1000", strict_rho=er, strict_u=eu, contracted_rho=cr, contracted_u=cu)


def test_c5_grid_16384x4096_fp32_single_gpu(lbm):
    """BASELINE.json configs[4] workload (16384x4096 fp32, Re=200) on ONE GPU (2.4 GB per population buffer; the 8-GPU
    strip run belongs to the driver), with the measured plan. The reference has no fp32 path and a CPU oracle run of 67 M
    cells is out of reach, so at full size the checks are the size-independent properties: geometry (130 721 solid
    cells), stability over 300 iterations, fp32 against this library's fp64 path on the same full-size grid at a
    stated, measured tolerance, run-to-run determinism,
    plan-to-plan bit-equality (measured plan vs LDS tiles vs the register kernel vs one launch per iteration) and
    decomposition invariance (8 in-process strips with the production exchange choreography == the whole domain)."""
    nx, ny, steps = 16384, 4096, 300
    kw = dict(inlet_velocity=0.01627604, precision="f32")

    def run(options):
        with lbm.Context(nx, ny, options=options, **kw) as ctx:
            assert ctx.initialise() == 130721
            ctx.step(steps, 150)
            assert ctx.first_unstable_step() == -1
            return ctx.macros(), ctx.drain_force_log(), ctx.plan(), ctx.kernel_name()
    (rho, ux, uy), log, plan, kernel = run(None)
    print("C5 plan:", plan, "|", kernel)
    assert np.isfinite(rho).all() and [r[0] for r in log] == [0, 150]
    # the yardstick at full size: this library's fp64 path on the same grid for the same 300 iterations (2 x 4.8 GB; it is
    # bit-identical to the oracle wherever the oracle reaches: 4096x1024 x 1000, 8192x2048 x 300). Stated tolerance: rho
    # 2e-5, u 2e-4, forces 1e-4 relative (L-inf / L-inf, u relative to max|u|); measured on MI355X (profiles/r03/
    # parity_measured.jsonl): rho 5.5e-6, u 3.1e-5, forces 1.7e-5 — the inlet velocity is 0.016, so ONE fp32 rounding of a
    # population (6e-8 of 0.44) already is 2e-6 of max|u|.
    with lbm.Context(nx, ny, inlet_velocity=0.01627604, precision="f64") as c64:
        assert c64.initialise() == 130721
        c64.step(steps, 150)
        assert c64.first_unstable_step() == -1
        m64 = c64.macros()
        log64 = c64.drain_force_log()
    er, eu = macro_errors(rho, ux, uy, *m64)
    ef = max(max(abs(a[1] - b[1]), abs(a[2] - b[2])) / abs(b[1]) for a, b in zip(log, log64))
    record("c5_16384x4096_f32_vs_hip_f64_300", rho=er, u=eu, force=ef, plan=plan)
    print(f"C5 fp32 vs fp64 (HIP) x {steps}: rho {er:.3e}, u {eu:.3e}, force {ef:.3e}")
    del m64
    assert er < 2e-5 and eu < 2e-4 and ef < 1e-4, (er, eu, ef)
    for options in (None, PLANS["rowil-fuse3-12-nt-xcd"], PLANS["rowil-col5-nt"], PLANS["rowil-deep6-nt"], PLANS["rowil-site-nt"], TALL_F32):
        m2, log2, _, _ = run(options)
        for a, b in zip((rho, ux, uy), m2):
            assert np.array_equal(a, b), options
        assert log2 == log
        del m2
    with lbm.Group(nx, ny, 8, options=dict(PLANS["rowil-fuse3-12-nt-xcd"]), **kw) as g:
        assert g.initialise() == 130721
        g.step(steps, 150)
        assert g.first_unstable_step() == -1
        for a, b in zip((rho, ux, uy), g.macros()):
            assert np.array_equal(a, b)
        glog = g.drain_force_log()
    for (t, fx, fy), (t2, gx, gy) in zip(log, glog):
        assert t == t2 and abs(fx - gx) <= 1e-6 * max(1.0, abs(fx)) and abs(fy - gy) <= 1e-6


def test_full_size_4096x1024_properties(lbm):
    """BASELINE.json configs[2] (headline size): 1000 iterations against the oracle (about 12 s of CPU on the GPU box's
    16 host threads), then run-to-run determinism across plans and strip-decomposition invariance, all bit for bit."""
    from oracle.oracle import Oracle, make_params
    nx, ny = 4096, 1024
    kw = dict(inlet_velocity=0.06510417)
    steps = 1000                      # parity window of the headline configuration
    o = Oracle(make_params(nx, ny, **kw))
    assert o.run(steps) == -1 and o.solid_count() == 8173
    with lbm.Context(nx, ny, **kw) as ctx:
        assert ctx.initialise() == 8173
        ctx.step(steps, 0)
        rho, ux, uy = ctx.macros()
        er, eu = macro_errors(rho, ux, uy, o.rho, o.ux, o.uy)
        assert er < TOL and eu < TOL, (er, eu)
        assert np.array_equal(ctx.populations("f_next"), o.f_next)      # bit-identical after 1000 iterations
        o_m = (o.rho.copy(), o.ux.copy(), o.uy.copy())      # (collide() moves the oracle's macros on to the next iteration)
        o.collide()
        fx, fy = ctx.forces()
        ofx, ofy = o.forces()
        assert abs(fx - ofx) <= TOL * abs(ofx) and abs(fy - ofy) <= TOL * abs(ofx)
        ctx.step(170, 0)
        assert ctx.first_unstable_step() == -1
        a = ctx.macros()
    # the bench's own mode: contracted arithmetic on ITS measured plan, the same 1000 iterations against the same oracle run
    with lbm.Context(nx, ny, options=dict(arith=1), **kw) as ctx:
        ctx.initialise()
        ctx.step(steps, 0)
        assert ctx.first_unstable_step() == -1
        cr, cu = macro_errors(*ctx.macros(), *o_m)
        fx, fy = ctx.forces()
        cf = max(abs(fx - ofx), abs(fy - ofy)) / abs(ofx)
        record("c3_4096x1024_f64_1000", strict_rho=er, strict_u=eu, contracted_rho=cr, contracted_u=cu, contracted_force=cf,
               contracted_plan=ctx.plan())
        print(f"C3 x {steps}: strict rho {er:.2e} u {eu:.2e} (populations bit-equal); contracted rho {cr:.2e} u {cu:.2e} F {cf:.2e} [{ctx.plan()}]")
        assert cr < TOL and cu < TOL and cf < TOL, (cr, cu, cf)
    o.close()
    with lbm.Context(nx, ny, options=PLANS["rowil-site-nt"], **kw) as ctx:   # a different plan, same bits
        ctx.initialise()
        ctx.step(steps + 170, 0)
        b = ctx.macros()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    ctxs, _ = _run_strips(lbm, nx, ny, [(0, 512), (512, 512)], 40, 0, **kw)
    with lbm.Context(nx, ny, **kw) as ctx:
        ctx.initialise()
        ctx.step(40, 0)
        w = ctx.macros()
    parts = [c.macros() for c in ctxs]
    for j in range(3):
        assert np.array_equal(np.concatenate([p[j] for p in parts], axis=0), w[j])
    for c in ctxs:
        c.close()
