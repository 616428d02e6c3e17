"""Time-averaged statistics on the GPU (lbm_stats_begin / k_stats): the six running sums a context accumulates on the device at the
force-output iterations of step(n, of) against the same sums formed on the host from a TWIN context's snapshots.

The sample of iteration t is defined as the (rho, ux, uy) `macros()` returns on a context with steps_done == t + 1. The twin has the
same parameters, plan and arithmetic; it does step(1) and macros() for t = 0, then step(of) and macros() for every later sample point,
and the test accumulates S = S + v, S = S + vx * vx, ... in numpy float64. Both sides perform the same IEEE operations on the same
doubles, so every comparison is np.array_equal: no tolerance is involved."""
import importlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.helpers import EXE, PKG, PLANS, TALL_F32, record, same_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lbm():
    pkg = importlib.import_module(PKG)
    assert pkg.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    assert hasattr(pkg.Context, "stats_begin")
    return pkg


NX, NY = 192, 72
KW = dict(inlet_velocity=0.06, cylinder_radius=0.12)
N, OF = 97, 10


def points(n, of, from_step=0, start=0):
    return [t for t in range(start, start + n) if of > 0 and t % of == 0 and t >= from_step]


def accumulate(S, snap):
    """one sample: S = S + v, each product rounded to double before it is added"""
    rho, ux, uy = snap
    S[0] = S[0] + rho
    S[1] = S[1] + ux
    S[2] = S[2] + uy
    S[3] = S[3] + ux * ux
    S[4] = S[4] + uy * uy
    S[5] = S[5] + ux * uy
    return S


def twin_sums(make, pts, S=None):
    """The expected sums: a fresh context from make() stepped to t + 1 for every sample point t, macros() there."""
    with make() as tw:
        tw.initialise()
        S = np.zeros((6, tw.local_ny, tw.nx)) if S is None else S.copy()
        for t in pts:
            tw.step(t + 1 - tw.steps_done)
            S = accumulate(S, tw.macros())
    return S


def run_stats(make, calls, from_step=0):
    with make() as c:
        c.initialise()
        c.stats_begin(from_step)
        for n, of in calls:
            c.step(n, of)
        return c.stats_sums(), c.stats_samples(), c.drain_force_log()


CALLS = [(5, OF), (20, OF), (N - 25, OF)]


# ---- plans and arithmetic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(PLANS))
def test_sums_equal_the_host_sums_of_the_twins_snapshots(lbm, plan):
    """Whole domain, fp64, strict and contracted, every plan of the parity suite; three calls of awkward lengths."""
    make = lambda: lbm.Context(NX, NY, options=PLANS[plan], **KW)
    got, n, log = run_stats(make, CALLS)
    pts = points(N, OF)
    assert n == len(pts) == len(log) and [r[0] for r in log] == pts
    assert np.array_equal(got, twin_sums(make, pts))


@pytest.mark.parametrize("plan", ["rowil-deep6-nt", "rowil-col5-nt", "fast-rowil-col6", "tall"])
def test_fp32_contexts_accumulate_in_double(lbm, plan):
    opts = TALL_F32 if plan == "tall" else PLANS[plan]
    make = lambda: lbm.Context(NX, NY, precision="f32", options=opts, **KW)
    got, n, _ = run_stats(make, CALLS)
    want = twin_sums(make, points(N, OF))
    assert n == 10 and np.array_equal(got, want)
    # the samples are floats widened to double: the sum of ten of them carries bits a float sum would not
    assert got.dtype == np.float64 and not np.array_equal(got[1], got[1].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("split", [3, 4])
def test_split_plans(lbm, split):
    """A whole-domain deep launch issued as row-range kernels on two streams: the sample follows the join."""
    opts = dict(tune=0, layout=1, pair_ty=12, xcd=1, deep=7, nt=1, alternate=0, arith=1, split=split, split_min=1)
    make = lambda: lbm.Context(512, 300, options=opts, inlet_velocity=0.08)
    got, n, _ = run_stats(make, CALLS)
    assert n == 10 and np.array_equal(got, twin_sums(make, points(N, OF)))


@pytest.mark.parametrize("nx", [191, 513, 66])
def test_odd_widths(lbm, nx):
    """An odd width takes the kernel's scalar path (the pairs of cells are not 16-byte aligned); 513 leaves a block with one cell."""
    make = lambda: lbm.Context(nx, 40, options=dict(tune=0, layout=1, fuse=1), inlet_velocity=0.05, cylinder_radius=0.1)
    got, n, _ = run_stats(make, [(31, 7)])
    assert n == 5 and np.array_equal(got, twin_sums(make, points(31, 7)))


# ---- features ------------------------------------------------------------------------------------------------------------------
def square(nx, ny):
    m = np.zeros((ny, nx), dtype=np.uint8)
    m[ny // 2 - 6:ny // 2 + 5, nx // 4:nx // 4 + 9] = 1
    m[3:7, nx // 2:nx // 2 + 30] = 1
    return m


@pytest.mark.parametrize("plan", ["rowil-site-nt", "fast-rowil-col6", "planar-deep7-alt"])
def test_obstacle_mask_inlet_profile_and_les(lbm, plan):
    mask = square(NX, NY)
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"])
    for kw in (dict(solid=mask), dict(inlet_profile=u), dict(smagorinsky=0.17), dict(solid=mask, inlet_profile=u, smagorinsky=0.17)):
        make = lambda: lbm.Context(NX, NY, options=PLANS[plan], **KW, **kw)
        with make() as c:
            solid_count = c.initialise()
            c.stats_begin(0)
            c.step(N, OF)
            got, n, st = c.stats_sums(), c.stats_samples(), c.stats()
        assert np.array_equal(got, twin_sums(make, points(N, OF)))
        if "solid" in kw:
            assert solid_count == int(mask.sum()) > 0
            s = mask.astype(bool)
            assert np.all(got[0][s] == n) and all(np.all(got[j][s] == 0.0) for j in range(1, 6))
            assert all(np.all(st[k][s] == 0.0) for k in ("uxux", "uyuy", "uxuy")) and np.all(st["rho"][s] == 1.0)


# ---- from_step -----------------------------------------------------------------------------------------------------------------
def test_from_step(lbm):
    make = lambda: lbm.Context(NX, NY, options=PLANS["fast-rowil-col6"], **KW)
    got, n, log = run_stats(make, CALLS, from_step=33)            # not on a sample point: 40, 50, .. 90
    assert n == 6 and len(log) == 10
    assert np.array_equal(got, twin_sums(make, points(N, OF, 33)))
    got, n, log = run_stats(make, CALLS, from_step=40)            # on one
    assert n == 6 and np.array_equal(got, twin_sums(make, points(N, OF, 40)))
    got, n, log = run_stats(make, CALLS, from_step=N + 5)         # beyond the end of the calls
    assert n == 0 and len(log) == 10 and not got.any()
    got, n, log = run_stats(make, [(N, 0)])                       # no output cadence: nothing is sampled
    assert n == 0 and log == [] and not got.any()


# ---- several calls -------------------------------------------------------------------------------------------------------------
def test_end_begin_and_the_sample_count(lbm):
    make = lambda: lbm.Context(NX, NY, options=PLANS["rowil-fuse3-12-nt-xcd"], **KW)
    with make() as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="never begun"):
            c.stats_sums()
        with pytest.raises(lbm.LbmError):
            c.stats_begin(-1)
        c.stats_begin(0)
        c.step(45, OF)
        assert c.stats_samples() == len(c.drain_force_log()) == 5
        kept = c.stats_sums()
        c.stats_end()
        c.step(30, OF)                                            # forces go on, samples do not
        assert len(c.drain_force_log()) == 3 and c.stats_samples() == 5
        assert np.array_equal(c.stats_sums(), kept)
        c.stats_begin(0)                                          # a second begin resets
        assert c.stats_samples() == 0 and not c.stats_sums().any()
        c.step(40, OF)                                            # 75 .. 114: samples at 80, 90, 100, 110
        assert c.stats_samples() == len(c.drain_force_log()) == 4
        got = c.stats_sums()
    assert np.array_equal(kept, twin_sums(make, [0, 10, 20, 30, 40]))
    assert np.array_equal(got, twin_sums(make, [80, 90, 100, 110]))
    with lbm.Context(NX, NY, **KW) as fresh:
        with pytest.raises(lbm.LbmError, match="initialised"):
            fresh.stats_begin(0)


def test_the_option_is_the_same_as_stats_begin(lbm):
    make = lambda: lbm.Context(NX, NY, options=PLANS["rowil-col5-nt"], **KW)
    with lbm.Context(NX, NY, options=dict(PLANS["rowil-col5-nt"], stats=20), **KW) as c:      # before initialise: begun at its end
        c.initialise()
        c.step(N, OF)
        a = c.stats_sums()
        assert c.stats_samples() == 8
        c.set_option("stats", 0)                                  # on an initialised context: lbm_stats_begin
        assert c.stats_samples() == 0 and not c.stats_sums().any()
    assert np.array_equal(a, twin_sums(make, points(N, OF, 20)))


# ---- groups --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap,deep_halo", [(1, 1), (2, 1), (1, 0), (2, 2), (0, 1)])
@pytest.mark.parametrize("plan", ["rowil-site-nt", "rowil-fuse3-12-nt-xcd", "rowil-deep6-nt", "fast-rowil-col6"])
@pytest.mark.parametrize("bounds", [[(0, 37), (37, 63)], [(0, 37), (37, 22), (59, 41)]])
def test_a_group_of_strips_accumulates_the_whole_domains_sums(lbm, bounds, plan, overlap, deep_halo):
    """Two and three strips on one device with the peer transport, boundaries on odd rows: the inlet and outlet cells of a strip's
    first and last row pull from a ghost row, which must hold the neighbour's P_t when the sample runs. Row for row the whole domain's
    sums — and those of the host loop over the whole domain's snapshots."""
    nx, ny, steps, of = 320, 100, 271, 45
    kw = dict(inlet_velocity=0.06, cylinder_radius=0.12)
    opts = dict(PLANS[plan], overlap=overlap, deep_halo=deep_halo, group_threads=0 if (overlap + deep_halo) % 2 else 1)
    make = lambda: lbm.Context(nx, ny, options=PLANS[plan], **kw)
    whole, n_whole, log = run_stats(make, [(5, of), (steps - 5, of)], from_step=1)
    with lbm.Group(nx, ny, bounds, options=opts, **kw) as g:
        g.initialise()
        g.stats_begin(1)
        g.step(5, of)
        g.step(steps - 5, of)
        assert g.first_unstable_step() == -1
        got, n = g.stats_sums(), g.stats_samples()
        st = g.stats()
        g.ctxs[0].stats_begin(0)                                  # one member reset on its own: the group must say so
        with pytest.raises(lbm.LbmError, match="disagree"):
            g.stats_samples()
    assert n == n_whole == 6 and got.shape == (6, ny, nx)
    assert np.array_equal(got, whole)
    assert np.array_equal(got, twin_sums(make, points(steps, of, 1)))
    assert st["n"] == 6 and np.array_equal(st["ux"], whole[1] / 6)


# ---- graph path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0])
def test_replayed_launch_groups_leave_the_sample_points_alone(lbm, overlap):
    """A loopback strip on a deep plan replays its launch groups from a captured graph between the force outputs; the samples sit at the
    force outputs, outside every replay: same sums as the twin (eager), same number of replays as without statistics."""
    nx, ny, steps, of = 512, 160, 437, 150
    base = dict(tune=0, layout=1, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, loopback=1, overlap=overlap)
    kw = dict(inlet_velocity=0.05, cylinder_radius=0.1)
    with lbm.Context(nx, ny, options=dict(base, graph=1), **kw) as c:
        c.initialise()
        c.stats_begin(0)
        c.step(steps, of)
        got, n, replays = c.stats_sums(), c.stats_samples(), c.graph_replays()
        f_with = c.populations("f_next")
    with lbm.Context(nx, ny, options=dict(base, graph=1), **kw) as c:
        c.initialise()
        c.step(steps, of)
        plain_replays = c.graph_replays()
        assert np.array_equal(c.populations("f_next"), f_with)
    assert n == 3 and replays == plain_replays > 0
    assert np.array_equal(got, twin_sums(lambda: lbm.Context(nx, ny, options=dict(base, graph=0), **kw), points(steps, of)))


# ---- restart -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [50, 53])
def test_a_restored_run_continues_its_averages(lbm, tmp_path, half):
    make = lambda: lbm.Context(NX, NY, options=PLANS["fast-rowil-col6"], **KW)
    whole, n_whole, _ = run_stats(make, [(N, OF)], from_step=15)
    with make() as a:
        a.initialise()
        a.stats_begin(15)
        a.step(half, OF)
        a.save_state(tmp_path / "s.ckpt")
        sums, n = a.stats_sums(), a.stats_samples()
    with make() as plain:                 # checkpoints do not carry statistics: the same bytes as a run without
        plain.initialise()
        plain.step(half, OF)
        plain.save_state(tmp_path / "p.ckpt")
    assert open(tmp_path / "s.ckpt", "rb").read() == open(tmp_path / "p.ckpt", "rb").read()
    with make() as b:
        b.initialise()
        b.stats_begin(15)
        b.load_state(tmp_path / "s.ckpt")                         # leaves the accumulators alone
        assert b.stats_samples() == 0
        b.stats_restore(sums, n)
        assert b.stats_samples() == n and np.array_equal(b.stats_sums(), sums)
        b.step(N - half, OF)
        assert b.stats_samples() == n_whole == 8
        assert np.array_equal(b.stats_sums(), whole)
    with make() as c:                     # restore on a context that never began: begins first, sampling active
        c.initialise()
        c.load_state(tmp_path / "s.ckpt")
        c.stats_restore(sums, n)
        c.step(N - half, OF)
        assert np.array_equal(c.stats_sums(), whole)
        with pytest.raises(ValueError):
            c.stats_restore(sums[:, 1:], n)


# ---- existing behaviour --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["auto", "rowil-col6-ntl-alt", "fast-rowil-fuse4-xcd"])
def test_statistics_change_nothing_else(lbm, plan):
    out = []
    for stats in (False, True):
        with lbm.Context(NX, NY, options=PLANS[plan], **KW) as c:
            c.initialise()
            if stats:
                c.stats_begin(0)
            for n, of in CALLS:
                c.step(n, of)
            out.append((c.populations("f_next"), c.populations("f_current"), c.drain_force_log(), c.first_unstable_step(), c.macros()))
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] == -1
    assert all(np.array_equal(u, v) for u, v in zip(a[4], b[4]))
    with lbm.Context(128, 32, tau=0.51, inlet_velocity=0.15, options=PLANS[plan]) as c, lbm.Context(128, 32, tau=0.51, inlet_velocity=0.15, options=PLANS[plan]) as d:
        c.initialise(); d.initialise()
        d.stats_begin(0)
        c.step(2000, 50); d.step(2000, 50)
        assert c.first_unstable_step() == d.first_unstable_step() >= 0


# ---- host ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--strips", "2"]])
def test_lbm_solver_writes_the_mean_fields(lbm, extra):
    base = ["--nx", "64", "--ny", "32", "--steps", "1201", "--output-frequency", "100", "--inlet-velocity", "0.04", "--cylinder-radius", "0.1",
            "--no-tune", "--no-vtk"] + extra
    d0, d1 = tempfile.mkdtemp(prefix="lbm_stats_"), tempfile.mkdtemp(prefix="lbm_stats_")
    p0 = subprocess.run([EXE] + base, cwd=d0, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    p1 = subprocess.run([EXE] + base + ["--stats-start", "400"], cwd=d1, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p0.returncode == 0 and p1.returncode == 0, (p0.stderr, p1.stderr)
    for name in ("forces.csv", "velocity_field.csv", "simulation_params.csv"):
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == ["mean_fields.csv", "mean_fields.vtk"]
    assert "mean_fields" not in p0.stdout and "Statistics" not in p0.stdout
    text = open(os.path.join(d1, "mean_fields.csv")).read()
    lines = text.splitlines()
    assert len(lines) == 1 + 64 * 32 and lines[0] == "x,y,rho,ux,uy,uxux,uyuy,uxuy"
    with lbm.Context(64, 32, inlet_velocity=0.04, cylinder_radius=0.1, options=dict(tune=0)) as c:
        c.initialise()
        c.stats_begin(400)
        c.step(1201, 100)
        st = c.stats()
    assert st["n"] == 9
    want = ["x,y,rho,ux,uy,uxux,uyuy,uxuy"]
    for y in range(32):
        for x in range(64):
            want.append(f"{x},{y}," + ",".join("%.8f" % st[k][y, x] for k in ("rho", "ux", "uy", "uxux", "uyuy", "uxuy")))
    same_text(text, "\n".join(want) + "\n")
    vtk = open(os.path.join(d1, "mean_fields.vtk")).read()
    assert "DATASET STRUCTURED_POINTS\nDIMENSIONS 64 32 1" in vtk and "VECTORS mean_velocity double" in vtk and "SCALARS reynolds_stress_uxuy double" in vtk
    assert len(vtk.splitlines()) == 9 + 64 * 32 + 4 * (3 + 64 * 32)


def test_lbm_solver_carries_the_sums_beside_a_checkpoint():
    base = ["--nx", "64", "--ny", "32", "--output-frequency", "100", "--inlet-velocity", "0.04", "--cylinder-radius", "0.1", "--no-tune", "--no-vtk",
            "--quiet", "--stats-start", "400", "--strips", "2"]
    d0, d1 = tempfile.mkdtemp(prefix="lbm_stats_"), tempfile.mkdtemp(prefix="lbm_stats_")
    subprocess.run([EXE] + base + ["--steps", "1201"], cwd=d0, check=True, timeout=300, stdout=subprocess.DEVNULL)
    subprocess.run([EXE] + base + ["--steps", "650", "--checkpoint", "s.ckpt", "--no-final"], cwd=d1, check=True, timeout=300, stdout=subprocess.DEVNULL)
    assert sorted(f for f in os.listdir(d1) if f.startswith("s.ckpt")) == ["s.ckpt.0", "s.ckpt.1", "s.ckpt.stats"]
    assert not [f for f in os.listdir(d1) if f.startswith("mean_fields")]      # --no-final: no partial averages beside the checkpoint
    subprocess.run([EXE] + base + ["--steps", "1201", "--restart", "s.ckpt"], cwd=d1, check=True, timeout=300, stdout=subprocess.DEVNULL)
    assert open(os.path.join(d0, "mean_fields.csv"), "rb").read() == open(os.path.join(d1, "mean_fields.csv"), "rb").read()
    os.remove(os.path.join(d1, "s.ckpt.stats"))           # a restart without the sums is not an error: the averages start afresh
    pr = subprocess.run([EXE] + base + ["--steps", "1201", "--restart", "s.ckpt"], cwd=d1, timeout=300, stdout=subprocess.PIPE, text=True)
    assert pr.returncode == 0 and "(6 samples)" in pr.stdout, pr.stdout


# ---- a physical sanity case ----------------------------------------------------------------------------------------------------
def test_a_steady_flow_has_no_reynolds_stresses(lbm):
    """256 x 64, the default cylinder, Re 20, strict arithmetic: the flow settles to a steady state, so the Reynolds stresses sampled
    over the second half of a long run must vanish against U^2. The bound 1e-6 is a SANITY FENCE, not a measurement: nobody has
    measured how small the residue is (it is printed and recorded here); a flow that really fluctuates at this regime — a shedding
    wake has u' of the order of 0.1 U — would exceed it by four orders of magnitude."""
    nx, ny, tau = 256, 64, 0.6
    d = 2.0 * int(0.05 * ny)
    u_in = 20.0 * ((tau - 0.5) / 3.0) / d
    # (the slowest channel mode decays like exp(-pi^2 nu t / ny^2) = e^-16 over the first half)
    steps, of = 400000, 200
    with lbm.Context(nx, ny, tau=tau, inlet_velocity=u_in, options=dict(arith=0), force_log_capacity=4096) as c:
        c.initialise()
        c.stats_begin(steps // 2)
        c.step(steps, of)
        assert c.first_unstable_step() == -1
        st = c.stats()
    assert st["n"] == steps // 2 // of
    worst = {k: float(np.max(np.abs(st[k]))) / u_in ** 2 for k in ("uxux", "uyuy", "uxuy")}
    print("max |<u'u'>| / U^2 over the second half of a steady Re 20 run:", worst)
    record("stats_steady_re20_256x64", samples=st["n"], **worst)
    assert max(worst.values()) < 1e-6, worst
