"""Periodic top and bottom boundaries (lbm_set_periodic_y) on the GPU: every kernel family a strip may run against the stepwise
reference of tests/periodic_reference.py on a lattice with a body across the seam, roll invariance, a uniform stream, groups of
strips on the ring against the lone periodic context, the combinations with the other features, the samplers, checkpoints and the
refusals that need a context."""
import functools

import numpy as np
import pytest

from tests.forcing_reference import guo_collide
from tests.helpers import (PLANS, U_BAR_ABS, assert_matches_reference, force_problems, lbm_gpu, macro_errors,  # noqa: F401
                           reference_problems, strict, u_bar_rel)
from tests.periodic_reference import (NX, NY, OF, STEPS, TAU, U0, periodic_run, read_only, seam_mask, seam_profile, seam_reference)
from tests.ports_reference import PRESSURE
from tests.reference import HOLD, les_collide, trt_collide

pytestmark = pytest.mark.gpu

KW = dict(tau=TAU, inlet_velocity=U0)
CALLS = [(13, OF), (1, OF), (20, OF), (26, OF)]          # 60 iterations in calls that end and begin launches at odd places
ROW = dict(tune=0, layout=1)
# one plan per kernel family a strip may run (a periodic context is a strip with two faces), strict and contracted
PERIODIC_PLANS = {
    "site": dict(ROW, nt=1, alternate=0),
    "site-alt-overlap0": dict(ROW, nt=0, alternate=1, overlap=0),
    "fuse2": dict(ROW, nt=0, alternate=1, pair=1, pair_ty=12, xcd=1),
    "fuse2-halo0": dict(ROW, nt=1, alternate=0, pair=1, pair_ty=8, deep_halo=0),
    "fuse3": dict(ROW, nt=1, alternate=0, fuse=3, pair_ty=12, xcd=1),
    "fuse3-overlap2": dict(ROW, nt=1, alternate=0, fuse=3, pair_ty=12, xcd=1, overlap=2),
    "fuse3-trim": dict(ROW, nt=1, alternate=0, fuse=3, pair_ty=8, halo_trim=1),
    "deep1": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=1),
    "deep1-pairs-trim": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=1, deep_halo=2, halo_trim=1),
    "deep2": dict(ROW, nt=0, alternate=1, pair_ty=8, xcd=0, deep=2),
    "deep3": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=3),
    "deep6": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=6),
    "deep7": dict(ROW, nt=0, alternate=1, pair_ty=8, xcd=1, deep=7),
    "deep7-pairs-overlap2": dict(ROW, nt=0, alternate=0, pair_ty=12, xcd=1, deep=7, deep_halo=2, overlap=2),
    "deep9": dict(ROW, nt=0, alternate=1, pair_ty=12, xcd=1, deep=9),
    "fast-site": dict(ROW, nt=1, alternate=0, fuse=1, arith=1),
    "fast-fuse3": dict(ROW, nt=1, alternate=0, fuse=3, pair_ty=12, xcd=1, arith=1),
    "fast-deep2": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=2, arith=1),
    "fast-deep7": dict(ROW, nt=1, alternate=0, pair_ty=12, xcd=1, deep=7, arith=1),
    "fast-deep9": dict(ROW, nt=0, alternate=0, pair_ty=12, xcd=1, deep=9, arith=1),
}
# fp32 contexts only: seven iterations on the tall 64x48 regions (the table of deep shapes lets a strip run them)
TALL_F32 = {0: dict(ROW, nt=0, alternate=1, pair_ty=12, xcd=1, deep=8), 1: dict(ROW, nt=0, alternate=1, pair_ty=12, xcd=1, deep=8, arith=1)}


def arith_of(name):
    return int(PERIODIC_PLANS[name].get("arith", 0))


def inputs(roll=0):
    return dict(solid=np.roll(seam_mask(), roll, axis=0), inlet_profile=np.roll(seam_profile(), roll))


def run_periodic(lbm, options, calls=CALLS, nx=NX, ny=NY, **kw):
    """(f_next, macros, force log, kernel name) of a periodic context after `calls`."""
    with lbm.Context(nx, ny, options=options, periodic_y=True, **kw) as ctx:
        ctx.initialise()
        assert ctx.periodic_y()
        for n, of in calls:
            ctx.step(n, of)
        assert ctx.first_unstable_step() == -1
        return ctx.populations("f_next"), ctx.macros(), ctx.drain_force_log(), ctx.kernel_name()


@functools.lru_cache(maxsize=None)
def lone(lbm, name, roll=0):
    """One run per plan and roll, shared (read-only) by the tests that hold other runs to it."""
    fn, macros, log, kernel = run_periodic(lbm, PERIODIC_PLANS[name], **KW, **inputs(roll))
    for a in (fn,) + tuple(macros):
        a.flags.writeable = False
    return fn, macros, log, kernel


# ---- 1. every family against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PERIODIC_PLANS))
def test_every_family_against_the_reference(lbm, name):
    """Strict plans: f_next bit for bit (the wrapped ghost rows and the zero ghost columns included), the forces across the seam at
    the force bar; contracted plans at the reference bars."""
    ref = seam_reference()
    assert ref.first_unstable == -1 and len(ref.forces) == STEPS // OF
    fn, macros, log, kernel = lone(lbm, name)
    o = PERIODIC_PLANS[name]
    want = "k_stepc_col" if o.get("deep", 0) >= 6 else "k_stepd_tile" if o.get("deep") else \
        "k_step3_tile" if o.get("fuse") == 3 else "k_step2_tile" if o.get("pair") else "k_step_site"
    assert kernel.startswith(want), (name, kernel)
    bad = reference_problems(arith_of(name), fn, macros, log, ref, u_bar_rel(ref))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def test_the_walls_are_gone(lbm):
    """The walled context on the same inputs differs on every row; the periodic reference is not the walled one."""
    walled = seam_reference(periodic=False)
    fn, _, _, _ = lone(lbm, "deep1")
    assert np.all(np.any(fn[1:-1, 1:-1] != walled.f_next[1:-1, 1:-1], axis=(1, 2)))
    with lbm.Context(NX, NY, options=PLANS["rowil-deep6-nt"], **KW, **inputs()) as w:
        w.initialise()
        for n, of in CALLS:
            w.step(n, of)
        assert not w.periodic_y()
        assert np.array_equal(w.populations("f_next"), walled.f_next)          # (without the call, what it was)


def test_fp32_tracks_the_fp64_reference(lbm):
    """fp32: one run per arithmetic against the fp64 reference at the fp32 bars of tests/test_gpu_parity.py (1e-3 relative on rho and
    u); every fp32 plan of one arithmetic gives the site plan's bits."""
    ref = seam_reference()
    for arith, names in ((0, ["site", "fuse3", "deep1", "deep7"]), (1, ["fast-site", "fast-fuse3", "fast-deep7"])):
        runs = [run_periodic(lbm, PERIODIC_PLANS[n], precision="f32", **KW, **inputs()) for n in names]
        runs.append(run_periodic(lbm, TALL_F32[arith], precision="f32", **KW, **inputs()))
        names = names + ["tall 64x48"]
        assert runs[-1][3].replace(" ", "").startswith("k_stepc_col<float,%s,7," % ("4,12" if arith else "6,8")), runs[-1][3]
        er, eu = macro_errors(*runs[0][1], ref.rho, ref.ux, ref.uy)
        print("fp32 arith %d against the fp64 reference: rho %.3g, u %.3g" % (arith, er, eu))
        assert er < 1e-3 and eu < 1e-3, (arith, er, eu)
        for n, r in zip(names[1:], runs[1:]):
            assert r[3].replace(" ", "").startswith(("k_stepc_col<float", "k_stepd_tile<float", "k_step3_tile<float")), (n, r[3])
            assert np.array_equal(r[0], runs[0][0]), n


# ---- 2. roll invariance, a uniform stream --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["deep1", "deep7", "fuse3", "fast-deep7", "fast-fuse3"])
def test_roll_invariance_on_the_device(lbm, name):
    """The same plan with mask and profile rolled by 17 rows gives the populations rolled by 17 rows, bit for bit: no row is special
    (tile boundaries and edge bands fall on other rows of the flow)."""
    a, _, la, _ = lone(lbm, name)
    b, _, lb, _ = lone(lbm, name, 17)
    assert np.array_equal(np.roll(a[1:-1], 17, axis=0), b[1:-1])
    assert not force_problems(lb, la)


@pytest.mark.parametrize("name", ["site", "deep1", "fast-deep7"])
def test_a_uniform_stream_stays_uniform(lbm, name):
    fluid = np.zeros((NY, NX), np.uint8)
    fn, (rho, ux, uy), _, _ = run_periodic(lbm, PERIODIC_PLANS[name], calls=[(STEPS, 0)], solid=fluid, **KW)
    assert np.all(fn[1:-1] == fn[1:2]) and np.all(rho == rho[0:1]) and np.all(ux == ux[0:1]) and np.all(uy == uy[0:1])
    with lbm.Context(NX, NY, options=PERIODIC_PLANS[name], solid=fluid, **KW) as w:
        w.initialise()
        w.step(STEPS, 0)
        wf = w.populations("f_next")
    assert not np.all(wf[1:-1] == wf[1:2])


# ---- 3. groups: the ring -----------------------------------------------------------------------------------------------------------------
def group_devices(lbm, transport, n):
    """Peer copies: every strip on device 0. RCCL creates one communicator per member together and wants distinct devices."""
    if transport == "peer":
        return [0] * n
    if lbm.device_count() < n:
        pytest.skip("an RCCL group needs one device per strip (%d here, %d strips)" % (lbm.device_count(), n))
    return list(range(n))


# (one host thread per strip, and on two plans the one-thread driver, which issues the same launches)
@pytest.mark.parametrize("name,threads", [("deep1", 1), ("fuse3", 1), ("site", 1), ("fast-deep7", 1), ("deep1-pairs-trim", 1), ("fuse3-overlap2", 1),
                                          ("deep1", 0), ("fuse3", 0)])
@pytest.mark.parametrize("bounds", [((0, 24), (24, 12), (36, 36)), ((0, 36), (36, 36)), ((0, 72),)])      # (a linked group of one: the lone context)
@pytest.mark.parametrize("transport", ["peer", "rccl"])
def test_group_strips_on_the_ring_are_the_lone_context(lbm, transport, bounds, name, threads):
    fn, macros, log, _ = lone(lbm, name)
    opts = dict(PERIODIC_PLANS[name], group_threads=threads)
    with lbm.Group(NX, NY, list(bounds), devices=group_devices(lbm, transport, len(bounds)), transport=transport, options=opts,
                   periodic_y=True, **KW, **inputs()) as g:
        g.initialise()
        for n, of in CALLS:
            g.step(n, of)
        assert g.first_unstable_step() == -1 and all(c.periodic_y() for c in g.ctxs)
        for u, v in zip(g.macros(), macros):
            assert np.array_equal(u, v)
        assert np.array_equal(g.populations("f_next")[1:-1], fn[1:-1])            # (interiors: the strips' rows)
        glog = g.drain_force_log()
        assert [r[0] for r in glog] == [r[0] for r in log]
        for (t, fx, fy), (_, wx, wy) in zip(glog, log):                           # (assert_group_is_whole's bar: sums in strip order)
            assert abs(fx - wx) <= 1e-13 * max(1.0, abs(wx)) and abs(fy - wy) <= 1e-13 * max(1.0, abs(wy))


@pytest.mark.parametrize("name", ["deep1", "deep7"])
def test_graph_replay_on_and_off_give_the_same_bits(lbm, name):
    out = {}
    for graph in (1, 0):
        with lbm.Context(NX, NY, options=dict(PERIODIC_PLANS[name], graph=graph), periodic_y=True, **KW, **inputs()) as ctx:
            ctx.initialise()
            ctx.step(150, 0)
            ctx.step(1, 0)
            out[graph] = (ctx.populations("f_next"), ctx.graph_replays())
    assert out[1][1] > 0 and out[0][1] == 0
    assert np.array_equal(out[1][0], out[0][0])


# ---- 4. combinations, on 192x48 ------------------------------------------------------------------------------------------------------------
CNX, CNY, CSTEPS, COF = 192, 48, 40, 10
CCALLS = [(17, COF), (23, COF)]


def combo_inputs():
    m = seam_mask(CNX, CNY)
    m[:, 150:] = 0
    return m, seam_profile(CNY)


SCHED = (np.linspace(0.4, 1.0, 25), HOLD)
COMBOS = {
    "les": (dict(smagorinsky=0.17, tau=0.53), dict(collide=functools.partial(les_collide, cs=0.17), tau=0.53)),
    "trt": (dict(trt_magic=3.0 / 16.0, tau=0.56), dict(collide=functools.partial(trt_collide, magic=3.0 / 16.0), tau=0.56)),
    "forcing": (dict(forcing=(0.0, 2e-5), tau=0.6), dict(collide=functools.partial(guo_collide, force=(0.0, 2e-5)), tau=0.6)),
    "pressure-pair": (dict(ports=((PRESSURE, 1.004), (PRESSURE, 0.996)), tau=0.6, profile=False),
                      dict(ports=((PRESSURE, 1.004), (PRESSURE, 0.996)), tau=0.6)),
    "schedule": (dict(inlet_schedule=(SCHED[0], "hold"), tau=0.6), dict(schedule=SCHED, tau=0.6)),
}


@functools.lru_cache(maxsize=None)
def combo_reference(combo):
    ctx_kw, ref_kw = COMBOS[combo]
    m, u = combo_inputs()
    return read_only(periodic_run(CNX, CNY, CSTEPS, COF, mask=m, u=u if ctx_kw.get("profile", True) else None, inlet_velocity=U0, **ref_kw))


@pytest.mark.parametrize("name", ["deep1", "fast-deep7"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_combinations_against_the_reference(lbm, combo, name):
    ctx_kw = dict(COMBOS[combo][0])
    profile = ctx_kw.pop("profile", True)
    m, u = combo_inputs()
    ref = combo_reference(combo)
    assert ref.first_unstable == -1
    fn, macros, log, _ = run_periodic(lbm, PERIODIC_PLANS[name], calls=CCALLS, nx=CNX, ny=CNY, solid=m, inlet_profile=u if profile else None,
                                      inlet_velocity=U0, **ctx_kw)
    # (tau near 0.5 amplifies: the absolute velocity bar of the LES and TRT tests; the forced snapshot adds F/2 on both sides)
    assert_matches_reference(arith_of(name), fn, macros, log, ref, U_BAR_ABS)


# ---- 5. the samplers -------------------------------------------------------------------------------------------------------------------------
def periodic_vorticity(ux, uy):
    """d uy/dx - d ux/dy with the central difference across the seam (np.roll in y); the x edges keep the one-sided form."""
    ddx = np.empty_like(uy)
    ddx[:, 1:-1] = 0.5 * (uy[:, 2:] - uy[:, :-2])
    ddx[:, 0] = uy[:, 1] - uy[:, 0]
    ddx[:, -1] = uy[:, -1] - uy[:, -2]
    return ddx - 0.5 * (np.roll(ux, -1, axis=0) - np.roll(ux, 1, axis=0))


@pytest.mark.parametrize("name", ["deep1", "fast-deep7"])
def test_statistics_frames_and_probes_across_the_seam(lbm, name):
    pts = [(0, 0), (77, 0), (NX - 1, 0), (39, NY - 1), (0, NY - 1), (NX - 1, NY - 1), (46, 3), (100.5, NY - 1), (12.25, 35.5)]
    snaps = {}
    for steps in (21, 41):                      # macros() after step(t + 1) is the snapshot the samplers take at t
        with lbm.Context(NX, NY, options=PERIODIC_PLANS[name], periodic_y=True, **KW, **inputs()) as twin:
            twin.initialise()
            twin.step(steps, 0)
            snaps[steps - 1] = twin.macros()
    with lbm.Context(NX, NY, options=PERIODIC_PLANS[name], periodic_y=True, frames=1, probes=np.array(pts, dtype=np.float64), **KW,
                     **inputs()) as ctx:
        ctx.initialise()
        ctx.stats_begin(20)
        ctx.step(41, 20)                        # statistics at t = 20 and 40; frames and probes at t = 0, 20, 40
        assert ctx.stats_samples() == 2
        sums = ctx.stats_sums()
        frames = ctx.drain_frames()
        ts, vals = ctx.drain_probes()
    (r1, x1, y1), (r2, x2, y2) = snaps[20], snaps[40]
    for got, want in zip(sums, (r1 + r2, x1 + x2, y1 + y2, x1 * x1 + x2 * x2, y1 * y1 + y2 * y2, x1 * y1 + x2 * y2)):   # a host loop over snapshots
        assert np.array_equal(got, want)
    assert [t for t, _ in frames] == [0, 20, 40] and list(ts) == [0, 20, 40]
    for (t, frame), (rho, ux, uy) in zip(frames[1:], (snaps[20], snaps[40])):
        for got, want in zip(frame[:3], (rho, ux, uy)):
            assert np.array_equal(got, want.astype(np.float32))
        ref = periodic_vorticity(ux, uy)
        for row in (0, NY - 1, 1, NY // 2):     # the wrapped central difference on rows 0 and ny - 1 (and two rows that never had another)
            err = float(np.max(np.abs(frame[3][row].astype(np.float64) - ref[row].astype(np.float32).astype(np.float64))))
            assert err <= 2.4e-7 * float(np.max(np.abs(ref))), (t, row, err)             # tests/test_gpu_frames.py BAR: two float32 ulps
        walled_row0 = (ref[0] + 0.5 * (ux[1] - ux[-1])) - (ux[1] - ux[0])                 # what the one-sided form would give
        assert float(np.max(np.abs(walled_row0 - ref[0]))) > 1e-6                        # (the two forms differ on this flow)
    for k, (rho, ux, uy) in ((1, snaps[20]), (2, snaps[40])):
        for j, (x, y) in enumerate(pts[:7]):    # probes on lattice points of rows 0 and ny - 1: those cells' macros
            assert np.array_equal(vals[k, j], np.array([rho[int(y), int(x)], ux[int(y), int(x)], uy[int(y), int(x)]])), (x, y)
        # between two columns of the last row: the two cells of that row, and no row beyond the seam
        mid = 0.5 * np.array([a[NY - 1, 100] + a[NY - 1, 101] for a in (rho, ux, uy)])
        assert np.allclose(vals[k, 7], mid, rtol=0, atol=1e-15), (vals[k, 7], mid)


def test_body_labels_away_from_the_seam_and_on_it(lbm):
    labels = np.zeros((NY, NX), np.uint8)
    labels[1:4, 40:46] = 1                      # next to the seam, not on it
    labels[NY // 2 - 2:NY // 2 + 2, 90:96] = 2
    labels[NY - 4:NY - 1, 120:124] = 3
    with lbm.Context(NX, NY, options=PERIODIC_PLANS["deep1"], periodic_y=True, bodies=labels, inlet_profile=seam_profile(), **KW) as ctx:
        ctx.initialise()
        ctx.step(30, 0)
        per_body = ctx.body_forces()
        total = ctx.forces()
    assert np.all(np.any(per_body != 0.0, axis=1))
    for k in range(2):
        assert abs(per_body[:, k].sum() - total[k]) <= 1e-13 * max(1.0, abs(total[k]))
    with lbm.Context(NX, NY, options=PERIODIC_PLANS["deep1"], periodic_y=True, solid=(labels != 0).astype(np.uint8), inlet_profile=seam_profile(),
                     **KW) as masked:
        masked.initialise()
        masked.step(30, 0)
        assert masked.forces() == total          # the masked total
    for row in (0, NY - 1):
        on = labels.copy()
        on[row, 10] = 4
        with lbm.Context(NX, NY, periodic_y=True, bodies=on, **KW) as bad:
            with pytest.raises(lbm.LbmError, match="body labels .* labelled cell on row %d beside periodic y" % row):
                bad.initialise()


# ---- 6. checkpoints ----------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_refusals(lbm, tmp_path):
    import struct
    fn, _, log, _ = lone(lbm, "deep1")
    path = tmp_path / "periodic.ckpt"
    with lbm.Context(NX, NY, options=PERIODIC_PLANS["deep7"], periodic_y=True, **KW, **inputs()) as a:
        a.initialise()
        a.step(30, OF)
        a.save_state(path)
    data = open(path, "rb").read()
    # magic, fixed header (72 bytes), flags (mask 1 | profile 2 | periodic y 512), the two digests; bit 9 has no payload
    assert data[:8] == b"LBMCKPT3" and struct.unpack("<Q", data[72:80]) == (1 | 2 | 512,) and len(data) == 96 + 9 * NX * NY * 8
    with lbm.Context(NX, NY, options=PERIODIC_PLANS["deep1"], periodic_y=True, **KW, **inputs()) as b:      # a fresh periodic context, another family
        b.initialise()
        b.load_state(path)
        b.step(29, OF)
        b.step(1, OF)
        assert np.array_equal(b.populations("f_next"), fn)                          # the uninterrupted run
        assert b.drain_force_log() == [r for r in log if r[0] >= 30]
    with lbm.Context(NX, NY, **KW, **inputs()) as walled:
        walled.initialise()
        with pytest.raises(lbm.LbmError, match="was written with periodic y; this context has two walls"):
            walled.load_state(path)
        walled.step(3, 0)
        walled.save_state(tmp_path / "walled.ckpt")
    with lbm.Context(NX, NY, periodic_y=True, **KW, **inputs()) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match=r"was written without periodic y \(two walls\); this context has periodic y"):
            c.load_state(tmp_path / "walled.ckpt")


# ---- 7. the refusals that need a context -------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_context(lbm):
    with lbm.Context(NX, NY, periodic_y=True, walls=("no-slip", "free-slip"), **KW) as c:
        with pytest.raises(lbm.LbmError, match="a no-slip south wall and a free-slip north wall .* beside periodic y"):
            c.initialise()
    with lbm.Context(NX, NY, periodic_y=True, walls=(("moving", 0.02), "no-slip"), **KW) as c:
        with pytest.raises(lbm.LbmError, match="a moving south wall and a no-slip north wall .* beside periodic y"):
            c.initialise()
    for opts, what in ((dict(tune=0, deep=10, arith=1), r"deep 10 .* exists for .* only"), (dict(tune=0, layout=0), "layout = 0 .* beside periodic y"),
                       (dict(tune=0, deep=11, arith=1), r"deep 11 .* exists for .* only"), (dict(tune=0, deep=7, split=3), "split = 3 beside periodic y"),
                       (dict(tune=0, loopback=1), "loopback = 1 .* beside periodic y")):
        with lbm.Context(NX, NY, periodic_y=True, options=opts, **KW) as c:
            with pytest.raises(lbm.LbmError, match=what):
                c.initialise()
    with lbm.Context(NX, NY, **KW) as c:
        for on in (2, -1):
            with pytest.raises(lbm.LbmError, match=r"lbm_set_periodic_y: on = %d \(0 or 1 only\)" % on):
                c.set_periodic_y(on)
        c.set_option("periodic_y", 1)
        assert c.periodic_y()
        c.set_periodic_y(0)                        # 0 clears
        assert not c.periodic_y()
    with lbm.Context(NX, 11, periodic_y=True, **KW) as c:
        with pytest.raises(lbm.LbmError, match="a strip of 11 rows beside periodic y"):
            c.initialise()
    with lbm.Context(NX, NY, periodic_y=True, **KW) as c:
        c.initialise()
        with pytest.raises(lbm.LbmError, match="lbm_set_periodic_y must be called before lbm_initialise"):
            c.set_periodic_y(False)
        with pytest.raises(lbm.LbmError, match="must be called before lbm_initialise"):
            c.set_option("periodic_y", 0)
        assert c.periodic_y()
        with pytest.raises(lbm.LbmError, match="lbm_halo_export: a periodic context"):
            c.halo_export()
        with pytest.raises(lbm.LbmError, match="lbm_halo_import: a periodic context"):
            c.halo_import(south=np.zeros((c.HALO_ROWS, 9, NX)), north=None)
        c.step(7, 0)                               # (a refusal leaves the context usable)
        assert c.first_unstable_step() == -1


def test_lbm_solver_runs_a_body_across_the_seam(lbm, tmp_path):
    """lbm_solver --periodic-y on one and on two strips: finite forces with a body across the seam, equal on both, and the line in
    simulation_params.csv."""
    import os
    import subprocess
    from tests.helpers import PKG, ROOT, read_csv_rows, read_params, run_solver, write_pgm
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, PKG, "host")])
    nx, ny = 256, 64
    m = np.zeros((ny, nx), np.uint8)
    m[ny - 4:, 50:58] = 1
    m[:4, 50:58] = 1
    write_pgm(tmp_path / "seam.pgm", m * 255)
    rows = {}
    for strips in (1, 2):
        d = tmp_path / ("s%d" % strips)
        d.mkdir()
        run_solver(["--nx", str(nx), "--ny", str(ny), "--steps", "200", "--output-frequency", "50", "--no-vtk", "--quiet", "--no-tune", "--periodic-y",
                    "--obstacle-mask", str(tmp_path / "seam.pgm"), "--strips", str(strips)], cwd=d)
        rows[strips] = [[float(v) for v in r] for r in read_csv_rows(d / "forces.csv")]
        assert len(rows[strips]) == 4 and np.all(np.isfinite(np.array(rows[strips])))
        assert read_params(d / "simulation_params.csv")["periodic_y"] == "1"
    assert np.allclose(np.array(rows[1]), np.array(rows[2]), rtol=0, atol=1e-12)
    assert abs(rows[1][-1][1]) > 1e-4               # drag on the body
