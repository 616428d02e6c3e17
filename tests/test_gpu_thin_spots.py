"""Round-4 parity tests for the three thin spots VERDICT r03 named (all through the C-ABI, all against the whole domain / the
oracle on the same inputs): (a) the PRODUCTION strip rule — k_stepc_col with one exchange per launch, options=None — at the
sizes the 8-GPU configurations name (8192x2048 fp64, 16384x4096 fp32) and on one 8192x256 strip with the one-rank RCCL transport
replayed from a hipGraph; (b) the exact calls the driver's bench makes at 4096x1024 (trailing_pair=1, step(5) then step(20) =
7+7+6) against the oracle; (c) fp32 held to 2 x the measured error instead of 10 x (tests/test_gpu_parity.py)."""
import importlib

import numpy as np
import pytest

from tests.helpers import PKG, macro_errors, record

pytestmark = pytest.mark.gpu
TOL = 1e-10      # north_star: rho / u within 1e-10 of the reference (L-inf / L-inf; u relative to max|u|)


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    pkg.build_all()
    if pkg.device_count() < 1:
        pytest.skip("no HIP device")
    return pkg


def moments(aos):
    """rho, ux, uy of an AoS population array [rows, nx+2, 9] (interior cells): the same numpy formula on both sides."""
    cx = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1.0])
    cy = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1.0])
    f = np.asarray(aos)[1:-1, 1:-1, :]
    rho = f.sum(axis=2)
    return rho, (f * cx).sum(axis=2) / rho, (f * cy).sum(axis=2) / rho


@pytest.mark.parametrize("arith", [0, 1])
def test_production_strip_rule_at_c4_size_8192x2048(lbm, arith):
    """Group(8192, 2048, 8) with no plan options: the rule's own pick for 256-row strips (k_stepc_col, six iterations per launch, ONE
    exchange per launch, schedule and store policy as measured) for 66 iterations + a force output == the whole domain bit for
    bit — in strict arithmetic and (round 5) in the CONTRACTED arithmetic an 8-GPU bench line would run.
    (Replaces Grid::exchange_ghost_cells, /root/reference/include/LBMGrid.h:249-283, between the strips.)"""
    nx, ny, steps, of = 8192, 2048, 66, 30
    kw = dict(inlet_velocity=0.03255208)
    opts = dict(arith=1) if arith else None
    with lbm.Context(nx, ny, options=opts, **kw) as whole:
        assert whole.initialise() == 32681
        whole.step(steps, of)
        assert whole.first_unstable_step() == -1
        w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
    with lbm.Group(nx, ny, 8, options=opts, **kw) as g:
        assert g.initialise() == 32681
        plans = [m.plan() for m in g.ctxs]
        assert all("6-step 64x32 in registers" in p for p in plans), plans
        assert all(m.kernel_name().startswith("k_stepc_col<double,4,8," if arith else "k_stepc_col<double,2,12,") for m in g.ctxs)
        schedule = g.ctxs[0].strip_schedule()
        g.step(steps, of)
        assert g.first_unstable_step() == -1
        assert np.array_equal(g.populations("f_next"), w_fn)
        log = g.drain_force_log()
    assert [r[0] for r in log] == [r[0] for r in w_log] == [0, 30, 60]
    for (t, fx, fy), (_, wx, wy) in zip(log, w_log):      # partial sums of the strips are added in another order
        assert abs(fx - wx) <= 1e-13 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-13
    record("c4_strips8_production_rule_66" + ("_contracted" if arith else ""), bit_equal=True, plan=plans[0], schedule=schedule)


@pytest.mark.parametrize("arith", [0, 1])
def test_production_strip_rule_at_c5_size_16384x4096_fp32(lbm, arith):
    """Group(16384, 4096, 8, precision='f32') with no plan options (512-row strips: k_stepc_col, one exchange per launch) for 66
    iterations == the whole domain, rho / ux / uy bit for bit (the populations of 67 M cells as fp64 AoS would be 2 x 4.8 GB of
    host memory; the snapshot is a function of the last two population states) — strict and, since round 5, contracted arithmetic
    (what `bench.py --gpus 8 --nx 16384 --ny 4096 --precision f32` runs)."""
    nx, ny, steps = 16384, 4096, 66
    kw = dict(inlet_velocity=0.01627604, precision="f32")
    opts = dict(arith=1) if arith else None
    with lbm.Context(nx, ny, options=opts, **kw) as whole:
        assert whole.initialise() == 130721
        whole.step(steps, 0)
        assert whole.first_unstable_step() == -1
        w = whole.macros()
    with lbm.Group(nx, ny, 8, options=opts, **kw) as g:
        assert g.initialise() == 130721
        plans = [m.plan() for m in g.ctxs]
        assert all("6-step 64x32 in registers" in p for p in plans), plans
        assert all(m.kernel_name().startswith("k_stepc_col<float,4,8,6,") for m in g.ctxs)
        g.step(steps, 0)
        assert g.first_unstable_step() == -1
        for a, b in zip(w, g.macros()):
            assert np.array_equal(a, b)
    record("c5_strips8_production_rule_66" + ("_contracted" if arith else ""), bit_equal=True, plan=plans[0])


def test_one_8192x256_strip_over_rccl_replayed_from_a_graph(lbm):
    """One 8192x256 strip (C4's strip height) that is its own north and south neighbour: the production RCCL exchange
    (ncclSend / ncclRecv on a one-rank communicator, loopback=2) on the rule's plan, issued eagerly and replayed from a hipGraph
    (four launch groups per replay), against device copies — populations bit for bit, and the graph path really ran."""
    nx, ny, steps = 8192, 256, 150
    kw = dict(inlet_velocity=0.03255208, cylinder_radius=0.1)
    out, replays = [], []
    for loopback, graph in ((1, 0), (2, 0), (2, 1)):
        with lbm.Context(nx, ny, options=dict(loopback=loopback, graph=graph), **kw) as ctx:
            if loopback == 2:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            assert "6-step 64x32 in registers" in ctx.plan(), ctx.plan()
            ctx.step(steps, 0)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
            out.append(ctx.populations("f_next"))
            replays.append(ctx.graph_replays())
    # (interior rows: the ghost rows of the previous iteration's buffer hold whatever the measured schedule last received into it)
    assert np.array_equal(out[0][1:-1], out[1][1:-1]) and np.array_equal(out[0][1:-1], out[2][1:-1])
    assert replays[0] == 0 and replays[1] == 0 and replays[2] > 0, replays


def test_the_drivers_own_calls_at_4096x1024_against_the_oracle(lbm):
    """bench.py --steps 20 --warmup 5 issues, on BASELINE.json configs[2]: lbm_step(5) then lbm_step(20) with trailing_pair=1 —
    on the register plan 5, then 7+7+6 (the seven-iteration kernel is a remainder depth of whole domains only). Both arithmetic
    modes after those 25 iterations (+ one single launch, so that the state can be read back) against the oracle: strict populations bit-equal; contracted (the bench's mode) rho / u of
    the populations within the north-star 1e-10. (/root/reference/include/LBMSolver.h:84-126 and :48-76.)"""
    from oracle.oracle import Oracle, make_params
    nx, ny = 4096, 1024
    kw = dict(inlet_velocity=0.06510417)
    o = Oracle(make_params(nx, ny, **kw))
    assert o.run(26) == -1
    o_fn = o.f_next.copy()
    o.close()
    o_m = moments(o_fn)
    for arith in (0, 1):
        with lbm.Context(nx, ny, options=dict(arith=arith, trailing_pair=1, timing=1), **kw) as ctx:
            ctx.initialise()
            ctx.step(5, 0)
            ctx.step(20, 0)
            _, launches, its = ctx.last_step_stats()
            kernel = ctx.kernel_name()
            assert ctx.first_unstable_step() == -1 and its == 20
            if "k_stepc_col" in kernel and ",6," in kernel:
                assert launches == 3, (kernel, launches)          # 7 + 7 + 6
            ctx.step(1, 0)          # (f_next is read from the previous iteration's buffer: one single-iteration launch makes it resident)
            fn = ctx.populations("f_next")
            if arith == 0:
                assert np.array_equal(fn, o_fn), kernel
            er, eu = macro_errors(*moments(fn), *o_m)
            ef = float(np.max(np.abs(fn - o_fn)))
            print(f"driver window, arith={arith} [{kernel}, {launches} launches]: rho {er:.2e} u {eu:.2e} max|df| {ef:.2e}")
            assert er < TOL and eu < TOL and ef < TOL, (arith, er, eu, ef)
            record(f"c3_driver_window_5_plus_20_arith{arith}", rho=er, u=eu, max_abs_df=ef, kernel=kernel, launches=launches)


def test_strict_div2_equals_ieee_division_in_its_range(lbm):
    """strict mode is 'IEEE op by op', but its two divisions by rho share one reciprocal chain without v_div_scale /
    v_div_fixup (csrc/lbm_kernels.hpp strict_div2). Held bit for bit against the compiler's own IEEE division on 4 M random
    operands of the documented range — denominators in [2^-20, 2^20] (rho ~ 1), numerators 0 or |a| in [2^-400, 2^400] — and
    the documented deviations outside it are what they are said to be (a -0 numerator gives +0)."""
    import ctypes
    L = ctypes.CDLL(lbm.lib_path())
    dp = ctypes.POINTER(ctypes.c_double)
    L.lbm_debug_strict_div2.argtypes = [dp, dp, dp, ctypes.c_int, dp, dp, dp, dp]
    rng = np.random.default_rng(20261004)
    n = 1 << 22

    def run(a1, a2, b):
        out = [np.empty(len(b)) for _ in range(4)]
        args = [np.ascontiguousarray(v, dtype=np.float64) for v in (a1, a2, b)]
        assert L.lbm_debug_strict_div2(*[v.ctypes.data_as(dp) for v in args], len(b), *[v.ctypes.data_as(dp) for v in out]) == 0
        return out

    def rand(lo, hi, size):      # magnitudes log-uniform over [2^lo, 2^hi], random sign
        return np.ldexp(rng.uniform(0.5, 1.0, size), rng.integers(lo + 1, hi + 1, size)) * rng.choice([-1.0, 1.0], size)

    b = np.abs(rand(-20, 20, n))
    b[: n // 2] = rng.uniform(1e-3, 1e1, n // 2)          # where the densities of a run live
    a1, a2 = rand(-400, 400, n), rand(-400, 400, n)
    a1[::7] = rng.uniform(-1.0, 1.0, len(a1[::7]))        # momenta of a run
    a2[::5] = 0.0
    q1, q2, r1, r2 = run(a1, a2, b)
    assert np.array_equal(q1.view(np.uint64), r1.view(np.uint64)) and np.array_equal(q2.view(np.uint64), r2.view(np.uint64))
    # outside the range: documented, not hidden
    q1, q2, r1, r2 = run(np.array([-0.0, 1.0]), np.array([0.0, 1.0]), np.array([1.5, 0.0]))
    assert q1[0] == 0.0 and not np.signbit(q1[0]) and np.signbit(r1[0])      # -0 / b: +0 here, -0 in IEEE
    assert np.isnan(q1[1]) and np.isinf(r1[1])                               # a / 0: NaN here, inf in IEEE (both flagged unstable)


@pytest.mark.parametrize("precision,ny,bounds,expect", [
    ("f64", 600, 3, "6-step 64x32 in registers"), ("f32", 600, 3, "6-step 64x32 in registers"), ("f64", 200, 3, "6-step 64x16"),
    ("f64", 600, [(0, 480), (480, 14), (494, 106)], "6-step 64x32 in registers")])
def test_deep_plans_in_pairs_over_a_twelve_row_halo(lbm, precision, ny, bounds, expect):
    """Round 4, "deep_halo" 2: a deep plan exchanges TWELVE rows per face once per TWO launches of six iterations — the first
    launch of a pair also updates the six ghost rows next to each internal face, redundantly with the neighbour (replaces
    Grid::exchange_ghost_cells, /root/reference/include/LBMGrid.h:249-283, at half the exchanges per iteration). Must reproduce
    the one-domain run bit for bit in every overlap mode, with one host thread per strip and with one for all, on even and on
    strongly uneven strips (a 14-row strip between tall ones), across force outputs that cut the pairs short."""
    nx, steps, of = 512, 333, 70
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1, precision=precision)
    ftol = 1e-13 if precision == "f64" else 1e-5        # partial force sums are added in a different order
    with lbm.Context(nx, ny, options=dict(tune=0, layout=1, nt=1, alternate=0, fuse=1), **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
    for extra in (dict(deep_halo=2), dict(deep_halo=2, overlap=0), dict(deep_halo=2, overlap=2), dict(deep_halo=2, group_threads=0)):
        with lbm.Group(nx, ny, bounds, options=extra, **kw) as g:
            g.initialise()
            assert all(expect in m.plan() for m in g.ctxs), [m.plan() for m in g.ctxs]
            g.step(steps, of)
            assert g.first_unstable_step() == -1
            fn = g.populations("f_next")
            rows = np.nonzero((fn != w_fn).any(axis=(1, 2)))[0]
            assert rows.size == 0, (extra, "rows that differ:", rows.tolist()[:40], "columns:", np.nonzero((fn != w_fn).any(axis=(0, 2)))[0].tolist()[:20],
                                    "populations:", np.nonzero((fn != w_fn).any(axis=(0, 1)))[0].tolist(), "max |d|", float(np.max(np.abs(fn - w_fn))))
            log = g.drain_force_log()
            assert [r[0] for r in log] == [r[0] for r in w_log]
            for (t, fx, fy), (_, wx, wy) in zip(log, w_log):
                assert abs(fx - wx) <= ftol * max(1.0, abs(wx)) and abs(fy - wy) <= ftol


@pytest.mark.parametrize("loopback", [1, 2])
def test_deep_pairs_on_one_strip_with_the_rccl_transport(lbm, loopback):
    """One strip that is its own neighbour (device copies / RCCL send-recv on a one-rank communicator): pairs of six-iteration
    launches over a twelve-row halo == one exchange of six rows per launch, bit for bit, overlapped and serialised; and a run
    that blows up reports the same first unstable iteration."""
    nx, ny = 512, 256
    base = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, loopback=loopback)
    for kw, steps, of in ((dict(inlet_velocity=0.05, cylinder_radius=0.1), 437, 150),
                          (dict(inlet_velocity=0.05, cylinder_radius=0.1, tau=0.5006), 700, 0)):        # the second one blows up
        out = []
        for sched in (dict(deep_halo=1, overlap=1, graph=0), dict(deep_halo=2, overlap=1, graph=0), dict(deep_halo=2, overlap=0, graph=0),
                      dict(deep_halo=2, overlap=2, graph=0), dict(deep_halo=2, overlap=1, graph=1), dict(deep_halo=2, overlap=0, graph=1)):
            with lbm.Context(nx, ny, options=dict(base, **sched), **kw) as ctx:
                if loopback == 2:
                    ctx.comm_init(0, 1, ctx.comm_unique_id())
                ctx.initialise()
                sd = ctx.strip_schedule()
                if sd and sched["deep_halo"] == 2:
                    assert "deep_halo=2" in sd and "12 iterations per exchange" in sd, sd
                ctx.step(steps, of)
                ctx.sync()
                bad = ctx.first_unstable_step()
                out.append((ctx.populations("f_next") if bad == -1 else None, ctx.drain_force_log(), bad))
                assert (ctx.graph_replays() > 0) == (sched["graph"] == 1), (sched, ctx.graph_replays(), ctx.strip_schedule())
        for other in out[1:]:
            assert out[0][2] == other[2] and out[0][1] == other[1]
            if out[0][0] is not None:      # (interior rows: the ghost rows of the previous iteration's buffer are whatever was last received into it)
                assert np.array_equal(out[0][0][1:-1], other[0][1:-1])
        assert (out[0][2] == -1) == (of == 150)


@pytest.mark.parametrize("deep,precision", [(3, "f64"), (2, "f64"), (3, "f32"), (9, "f64")])
def test_seven_and_eight_iteration_lds_shapes_on_strips(lbm, deep, precision):
    """Round 4: with the twelve-row ghost frame the seven- / eight-iteration LDS shapes (k_stepd_tile 64x16 x 7, 32x32 x 8) run on
    strips too, and so does the register kernel with seven iterations as its plan's depth ("deep" 9) — the exchange then refreshes seven / eight rows per face once per launch (fewer exchanges per iteration: one rank
    of eight, 7.36 -> 6.78 us per iteration in the proxy). Groups of even and uneven strips, every overlap mode, device copies
    and the RCCL loopback, eager and graph-replayed: bit-identical to the one-domain run."""
    nx, ny, steps, of = 512, 300, 333, 70
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1, precision=precision)
    ftol = 1e-13 if precision == "f64" else 1e-5
    plan = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=deep)
    with lbm.Context(nx, ny, options=dict(tune=0, layout=1, nt=1, alternate=0, fuse=1), **kw) as whole:
        whole.initialise()
        whole.step(steps, of)
        w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
    for bounds in (3, [(0, 150), (150, 14), (164, 136)]):
        for extra in (dict(), dict(overlap=0), dict(group_threads=0)):
            with lbm.Group(nx, ny, bounds, options=dict(plan, **extra), **kw) as g:
                g.initialise()
                assert all(f",{8 if deep == 3 else 7}," in m.kernel_name() and ("k_stepc_col" if deep == 9 else "k_stepd_tile") in m.kernel_name()
                           for m in g.ctxs), g.ctxs[0].kernel_name()
                g.step(steps, of)
                assert g.first_unstable_step() == -1
                assert np.array_equal(g.populations("f_next"), w_fn), (bounds, extra)
                log = g.drain_force_log()
                assert [r[0] for r in log] == [r[0] for r in w_log]
                for (t, fx, fy), (_, wx, wy) in zip(log, w_log):
                    assert abs(fx - wx) <= ftol * max(1.0, abs(wx)) and abs(fy - wy) <= ftol
    out = []
    for loopback, overlap, graph, d in ((1, 1, 0, 1), (1, 1, 0, deep), (2, 1, 0, deep), (2, 0, 0, deep), (2, 1, 1, deep)):
        with lbm.Context(nx, 160, options=dict(plan, deep=d, loopback=loopback, overlap=overlap, graph=graph), **kw) as ctx:
            if loopback == 2:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            ctx.step(steps, 160)      # (four launch groups of eight iterations are replayed only far from a force output)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
            out.append((ctx.populations("f_next")[1:-1], ctx.drain_force_log()))
            assert (ctx.graph_replays() > 0) == (graph == 1), ctx.strip_schedule()
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][1] == other[1]


@pytest.mark.parametrize("arith", [0, 1])
def test_tall_fp32_regions_in_registers(lbm, arith):
    """Round 4, fp32 only ("deep" 8): k_stepc_col on 64x48 regions (contracted arithmetic: twelve waves x four rows; strict: eight x six) with
    seven iterations per launch and six / eight for what a segment leaves over — the measured plan of 16384x4096 fp32. Same
    per-cell operation sequence as one launch per iteration: bit-identical populations and forces on ragged grids with every
    boundary and the cylinder (on the inlet column too), as a whole domain, as groups of even / uneven strips (seven rows per
    exchange), over the one-rank RCCL transport, eager and replayed from a graph. fp64 contexts refuse the shape."""
    with pytest.raises(lbm.LbmError, match="fp32 only"):
        lbm.Context(256, 64, precision="f64", options=dict(tune=0, deep=8))
    shape = "4,12" if arith else "6,8"      # rows per thread, waves per block
    site = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=arith)
    tall = dict(tune=0, layout=1, nt=0, alternate=1, pair_ty=12, xcd=1, deep=8, arith=arith)
    for (nx, ny, steps, of, kw) in ((300, 170, 333, 45, dict(inlet_velocity=0.05, cylinder_radius=0.1)),
                                    (1024, 256, 200, 0, dict(inlet_velocity=0.1)),
                                    (190, 140, 150, 31, dict(inlet_velocity=0.04, cylinder_x=0.02, cylinder_radius=0.12))):
        kw = dict(kw, precision="f32")
        with lbm.Context(nx, ny, options=site, **kw) as whole:
            whole.initialise()
            whole.step(steps, of)
            w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
        for extra in (dict(), dict(trailing_pair=1), dict(layout=0, alternate=0)):
            with lbm.Context(nx, ny, options=dict(tall, timing=1, **extra), **kw) as ctx:
                ctx.initialise()
                assert f"k_stepc_col<float,{shape},7,false,{arith}>" == ctx.kernel_name().replace(" ", ""), ctx.kernel_name()
                ctx.step(steps, of)
                if extra.get("trailing_pair"):
                    ctx.step(1, 0)
                    with lbm.Context(nx, ny, options=site, **kw) as w1:
                        w1.initialise()
                        w1.step(steps, of)
                        w1.step(1, 0)
                        ref_fn = w1.populations("f_next")
                else:
                    ref_fn = w_fn
                assert ctx.first_unstable_step() == -1
                assert np.array_equal(ctx.populations("f_next"), ref_fn), (nx, ny, extra)
                assert ctx.drain_force_log() == w_log
        if ny < 170:
            continue
        for bounds in (2, [(0, ny - 100), (ny - 100, 14), (ny - 86, 86)]):
            for extra in (dict(), dict(overlap=0, group_threads=0)):
                with lbm.Group(nx, ny, bounds, options=dict(tall, **extra), **kw) as g:
                    g.initialise()
                    assert all(f"<float,{shape},7," in m.kernel_name().replace(" ", "") for m in g.ctxs), g.ctxs[0].kernel_name()
                    g.step(steps, of)
                    assert g.first_unstable_step() == -1
                    assert np.array_equal(g.populations("f_next"), w_fn), (nx, ny, bounds, extra)
                    log = g.drain_force_log()
                    assert [r[0] for r in log] == [r[0] for r in w_log]
                    for (t, fx, fy), (_, wx, wy) in zip(log, w_log):
                        assert abs(fx - wx) <= 1e-5 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-5
    out = []
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1, precision="f32")
    for loopback, overlap, graph, d in ((1, 1, 0, 7), (1, 1, 0, 8), (2, 1, 0, 8), (2, 0, 0, 8), (2, 1, 1, 8)):
        with lbm.Context(512, 200, options=dict(tall, deep=d, loopback=loopback, overlap=overlap, graph=graph), **kw) as ctx:
            if loopback == 2:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            ctx.step(333, 160)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
            out.append((ctx.populations("f_next")[1:-1], ctx.drain_force_log()))
            assert (ctx.graph_replays() > 0) == (graph == 1), ctx.strip_schedule()
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][1] == other[1]


def test_the_fp32_kernel_of_the_bench_line_at_its_own_size_and_mode(lbm):
    """the driver's fp32 line (BASELINE.json configs[4] on one GPU) reports k_stepc_col<float,4,12,7,false,1> —
    CONTRACTED arithmetic, twelve waves x four rows, seven iterations per launch — at 16384x4096, and until round 5 every full-size
    fp32 test ran strict arithmetic. Here: that kernel (pinned, name asserted; and whatever options=dict(arith=1) measures, which
    must agree with it bit for bit) for 300 iterations against this library's fp64 CONTRACTED path on the same grid at the stated
    2e-5 (rho) / 2e-4 (u) / 1e-4 (forces), and bit-equal to one contracted k_step_site launch per iteration on the same grid
    (300 iterations, two force outputs; and a 21-iteration call = 7+7+6+1). What it must reproduce: collision_step,
    /root/reference/include/LBMSolver.h:84-126, in single precision (the reference has no fp32 path)."""
    nx, ny, steps = 16384, 4096, 300
    kw = dict(inlet_velocity=0.01627604, precision="f32")
    tall = dict(tune=0, layout=1, nt=0, alternate=1, pair_ty=12, xcd=1, deep=8, arith=1)
    site = dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=1)

    def run(options, n, of):
        with lbm.Context(nx, ny, options=options, **kw) as ctx:
            assert ctx.initialise() == 130721
            ctx.step(n, of)
            assert ctx.first_unstable_step() == -1
            return ctx.macros(), ctx.drain_force_log(), ctx.plan(), ctx.kernel_name().replace(" ", "")
    m_tall, log_tall, _, k_tall = run(tall, steps, 150)
    assert k_tall == "k_stepc_col<float,4,12,7,false,1>", k_tall
    m_auto, log_auto, plan_auto, k_auto = run(dict(arith=1), steps, 150)
    print("C5 contracted, measured plan:", plan_auto, "|", k_auto)
    assert k_auto.startswith("k_stepc_col<float,") and k_auto.endswith(",1>"), k_auto
    for a, b in zip(m_tall, m_auto):
        assert np.array_equal(a, b)
    assert log_auto == log_tall
    del m_auto
    m_site, log_site, _, k_site = run(site, steps, 150)
    assert k_site == "k_step_site<float,0,true,1>", k_site
    for a, b in zip(m_tall, m_site):
        assert np.array_equal(a, b)
    assert log_site == log_tall
    del m_site
    (a21, l21, _, _), (b21, m21, _, _) = run(tall, 21, 0), run(site, 21, 0)
    for a, b in zip(a21, b21):
        assert np.array_equal(a, b)
    del a21, b21
    with lbm.Context(nx, ny, inlet_velocity=0.01627604, precision="f64", options=dict(arith=1)) as c64:
        assert c64.initialise() == 130721
        c64.step(steps, 150)
        assert c64.first_unstable_step() == -1
        m64, log64 = c64.macros(), c64.drain_force_log()
    er, eu = macro_errors(*m_tall, *m64)
    ef = max(max(abs(a[1] - b[1]), abs(a[2] - b[2])) / abs(b[1]) for a, b in zip(log_tall, log64))
    record("c5_16384x4096_f32_contracted_tall_vs_hip_f64_contracted_300", rho=er, u=eu, force=ef, kernel=k_tall, measured_plan=plan_auto)
    print(f"C5 fp32 contracted (tall regions) vs fp64 contracted (HIP) x {steps}: rho {er:.3e}, u {eu:.3e}, force {ef:.3e}")
    assert er < 2e-5 and eu < 2e-4 and ef < 1e-4, (er, eu, ef)


def test_fp32_contracted_plans_agree_bit_for_bit_at_1024x256(lbm):
    """The link VERDICT r04 (weak 1a) found unasserted: in fp32 CONTRACTED arithmetic plan-independence was held tall <-> site only,
    while the oracle bound (2e-4 after 1000 iterations, tests/test_gpu_parity.py) is asserted on the MEASURED plan. Here, at
    1024x256 x 1000: measured plan == one launch per iteration == tall regions == 64x32 regions == LDS tiles, populations bit for bit."""
    nx, ny, steps = 1024, 256, 1000
    kw = dict(inlet_velocity=0.13020833, precision="f32")
    plans = {"auto": dict(arith=1), "site": dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=1),
             "tall": dict(tune=0, layout=1, nt=0, alternate=1, pair_ty=12, xcd=1, deep=8, arith=1),
             "col6": dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, arith=1),
             "lds8": dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=3, arith=1),
             "tile3": dict(tune=0, layout=1, nt=1, alternate=0, fuse=3, pair_ty=12, xcd=1, arith=1)}
    out = {}
    for name, options in plans.items():
        with lbm.Context(nx, ny, options=options, **kw) as ctx:
            assert ctx.initialise() == 441
            ctx.step(steps, 0)
            assert ctx.first_unstable_step() == -1
            out[name] = (ctx.populations("f_next"), ctx.kernel_name().replace(" ", ""))
    assert out["tall"][1] == "k_stepc_col<float,4,12,7,false,1>" and out["site"][1] == "k_step_site<float,0,true,1>"
    print("fp32 contracted 1024x256, measured plan:", out["auto"][1])
    for name, (fn, kernel) in out.items():
        assert np.array_equal(fn, out["site"][0]), (name, kernel)


def test_the_trimmed_halo_message_is_result_invariant(lbm):
    """Option "halo_trim" 1 (round 5, VERDICT r04 #7a): an exchange carries 9 hr - 9 of the 9 hr sub-rows of a face, in five messages
    — what tests/test_cabi_cpu.py derives from the dependency cone. The sub-rows that never travel go stale; no valid cell may read
    them: groups of three uneven strips (peer copies) on every frame depth the schedules use — six rows (three-iteration pairs, the
    six-iteration LDS and register shapes), seven ("deep" 9), eight ("deep" 3), twelve ("deep_halo" 2) — across force outputs == the
    whole domain bit for bit, and one strip over the one-rank RCCL transport, eager and replayed from a graph, == untrimmed.
    (Replaces pack_data_for_sending / unpack_received_data, /root/reference/include/LBMGrid.h:395-491, which move all nine values.)"""
    nx, ny, steps, of = 320, 300, 233, 50
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    bounds = [(0, 130), (130, 40), (170, 130)]
    for arith in (0, 1):
        with lbm.Context(nx, ny, options=dict(tune=0, layout=1, nt=1, alternate=0, fuse=1, arith=arith), **kw) as whole:
            whole.initialise()
            whole.step(steps, of)
            w_fn, w_log = whole.populations("f_next"), whole.drain_force_log()
        for plan in (dict(fuse=3, pair_ty=12, deep_halo=1), dict(fuse=3, pair_ty=8, deep_halo=0), dict(deep=1, deep_halo=1), dict(deep=7, deep_halo=1), dict(deep=7, deep_halo=2),
                     dict(deep=6, deep_halo=2), dict(deep=9, deep_halo=1), dict(deep=3, deep_halo=1), dict(deep=2, deep_halo=1)):
            for overlap in (0, 1, 2):
                opts = dict(tune=0, layout=1, nt=1, alternate=0, xcd=1, arith=arith, overlap=overlap, halo_trim=1, **plan)
                with lbm.Group(nx, ny, bounds, options=opts, **kw) as g:
                    g.initialise()
                    g.step(steps, of)
                    assert g.first_unstable_step() == -1
                    assert np.array_equal(g.populations("f_next"), w_fn), opts
                    assert [r[0] for r in g.drain_force_log()] == [r[0] for r in w_log]
    out = []
    for trim, loopback, overlap, graph, deep in ((0, 1, 0, 0, 7), (1, 1, 1, 0, 7), (1, 2, 1, 0, 7), (1, 2, 1, 1, 7), (1, 2, 0, 1, 7)):
        with lbm.Context(512, 200, options=dict(tune=0, layout=1, nt=1, alternate=0, xcd=1, deep=deep, arith=1, loopback=loopback, overlap=overlap, graph=graph,
                                                halo_trim=trim, deep_halo=1), **kw) as ctx:
            if loopback == 2:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            ctx.initialise()
            ctx.step(333, 160)
            ctx.sync()
            assert ctx.first_unstable_step() == -1
            sched = ctx.strip_schedule()
            assert f"halo_trim={trim}" in sched and (f"{(54 - 9 * trim) * 544 * 8} B per face and exchange" in sched), sched
            assert (ctx.graph_replays() > 0) == (graph == 1), sched
            out.append((ctx.populations("f_next")[1:-1], ctx.drain_force_log()))
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and out[0][1] == other[1]


def test_kernel_name_is_the_kernel_that_really_runs_on_a_host_staged_strip(lbm):
    """a strip whose halos are staged through the host carries LBM_HALO_ROWS = 6 ghost rows per exchange, so a plan of seven
    or eight iterations per launch falls back to the three-iteration tile kernel there (plan_launch) — and lbm_kernel_name must say so,
    because bench.py attributes time and counter bytes by that name. Whole domains and strips with a device transport keep the plan's
    own kernel."""
    kw = dict(inlet_velocity=0.05)
    with lbm.Context(256, 120, y_start=40, local_ny=40, options=dict(tune=0, layout=1, nt=0, pair_ty=12, xcd=1, deep=9, arith=1), **kw) as strip:
        strip.initialise()
        assert strip.kernel_name().replace(" ", "") == "k_step3_tile<double,12,1024,1>", strip.kernel_name()
    with lbm.Context(256, 120, options=dict(tune=0, layout=1, nt=0, pair_ty=12, xcd=1, deep=9, arith=1), **kw) as whole:
        whole.initialise()
        assert whole.kernel_name().replace(" ", "") == "k_stepc_col<double,4,8,7,false,1>", whole.kernel_name()
    with lbm.Context(256, 40, options=dict(tune=0, layout=1, nt=0, pair_ty=12, xcd=1, deep=9, arith=1, loopback=1), **kw) as loop:
        loop.initialise()
        assert loop.kernel_name().replace(" ", "") == "k_stepc_col<double,4,8,7,false,1>", loop.kernel_name()
    with lbm.Context(256, 120, y_start=40, local_ny=40, options=dict(tune=0, layout=1, nt=1, pair_ty=12, xcd=1, deep=7, arith=1), **kw) as six:
        six.initialise()       # six iterations per launch fit the six staged rows: the register kernel stays
        assert six.kernel_name().replace(" ", "") == "k_stepc_col<double,4,8,6,true,1>", six.kernel_name()



@pytest.mark.timeout(600)
def test_bench_dump_outputs_hold_the_last_timed_iteration(lbm, tmp_path):
    """bench.py --dump-outputs after `--steps 20 --warmup 5` (trailing_pair=1: the call may end on a fused launch) writes the
    post-collision populations of the 25th step, read through lbm_save_state — the oracle's f_next after 26 iterations, since a step
    of the library ends on the collision the oracle's next iteration begins with (lbm_initialise collides once): strict arithmetic
    bit-equal at every site of a grid small enough to be dumped whole, contracted within the north-star 1e-10."""
    import json
    import os
    import subprocess
    import sys
    from oracle.oracle import Oracle, make_params
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nx, ny, re_number = 256, 64, 10.0
    u_in = re_number * ((0.6 - 0.5) / 3.0) / (2.0 * 0.05 * ny)      # bench.py's u_in for --re
    o = Oracle(make_params(nx, ny, inlet_velocity=u_in))
    assert o.run(26) == -1
    ref = np.ascontiguousarray(o.f_next[1:-1, 1:-1, :].transpose(2, 0, 1)).reshape(9, nx * ny)
    o.close()
    for arith in ("strict", "contracted"):
        d = tmp_path / arith
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--nx", str(nx),
                              "--ny", str(ny), "--re", str(re_number), "--arith", arith, "--dump-outputs", str(d)],
                             cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 20 and line["ms_per_step"] > 0 and "sustained" not in line
        pops, sites = np.load(d / "populations.npy"), np.load(d / "sites.npy")
        assert pops.dtype == np.float64 and pops.shape == (9, nx * ny) and np.array_equal(sites, np.arange(nx * ny))
        if arith == "strict":
            assert np.array_equal(pops, ref), line["config"]["kernel"]
        err = float(np.max(np.abs(pops - ref)))
        assert err < TOL, (arith, err, line["config"]["kernel"])
