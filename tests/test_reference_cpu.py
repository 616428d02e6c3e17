"""tests/reference.py against the unmodified C oracle (no GPU): each shared piece, switched on in a way that must change nothing, gives
the plain run's bits — also under another feature — and the stepwise loop, whose boundary step is numpy, gives those of Oracle.run. A
later edit of the shared moment, equilibrium, boundary or loop code therefore cannot move every feature's reference at once without
failing here."""
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle, make_params
from tests.helpers import assert_forces_match, square
from tests.reference import FREESLIP, HOLD, NOSLIP, les_collide, moving, oracle_run, trt_collide

NX, NY, STEPS, OF = 160, 48, 120, 30
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
GEOMETRIES = ["disc", "square"]


def mask_of(geometry):
    return square(NX, NY) if geometry == "square" else None


@functools.lru_cache(maxsize=None)
def plain(geometry):
    """oracle_run with nothing switched on: computed once per geometry, shared, left unchanged."""
    return oracle_run(NX, NY, STEPS, OF, mask=mask_of(geometry), **KW)


def assert_same_run(got, want):
    for name in ("f_next", "rho", "ux", "uy"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.forces == want.forces and [r[0] for r in got.forces] == [0, 30, 60, 90]
    assert got.first_unstable == want.first_unstable == -1
    assert np.all(np.isfinite(got.f_next)) and np.max(np.abs(got.uy)) > 1e-6      # a flow, not a state at rest


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_les_collide_with_cs_zero_is_the_oracles_collision(geometry):
    """tau_eff = 0.5 (tau + sqrt(tau^2)) = tau exactly: the shared moments, feq and write-back are lbmo_collide's, bit for bit."""
    got = oracle_run(NX, NY, STEPS, OF, mask=mask_of(geometry), collide=functools.partial(les_collide, cs=0.0), **KW)
    assert_same_run(got, plain(geometry))
    assert got.tau_max == KW["tau"] and plain(geometry).tau_max is None


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_a_constant_profile_is_the_uniform_inlet(geometry):
    """feq_rows and the per-row inlet block with u[y] = u_in on every row are feq_init and the oracle's own inlet."""
    got = oracle_run(NX, NY, STEPS, OF, mask=mask_of(geometry), u=np.full(NY, KW["inlet_velocity"]), **KW)
    assert_same_run(got, plain(geometry))


def test_the_discs_own_cells_as_a_mask_are_the_disc():
    o = Oracle(make_params(NX, NY, **KW))
    o.L.lbmo_initialise(o.h)
    solid = o.solid.copy()
    o.close()
    got = oracle_run(NX, NY, STEPS, OF, mask=solid, **KW)
    assert_same_run(got, plain("disc"))
    assert got.solid_count == plain("disc").solid_count == int(solid.sum()) > 0


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_the_stepwise_loop_is_oracle_run(geometry):
    """Populations and macros bit for bit. The force rows of Oracle.run come from lbmo_forces, those of oracle_run from the numpy
    link_forces: the same links summed in another order, so they are held to the bar the GPU tests use for oracle forces,
    1e-10 * max(1, |F|), not to equality (measured: at most 7.7e-16 absolute). lbmo_forces sums over the links of the analytic disc
    whatever the mask (on the square it reports Fx = 8.80 at t = 0 where the square's links give 3.36), so the square compares the
    timesteps of its rows only."""
    o = Oracle(make_params(NX, NY, **KW))
    if geometry == "square":
        o.solid[:] = square(NX, NY)
    o.L.lbmo_initialise(o.h)
    rows = []
    bad = o.run(STEPS, OF, rows)
    want = plain(geometry)
    for name in ("f_next", "rho", "ux", "uy"):
        assert np.array_equal(getattr(o, name), getattr(want, name)), name
    assert bad == want.first_unstable == -1 and o.solid_count() == want.solid_count
    o.close()
    assert [r[0] for r in rows] == [r[0] for r in want.forces] == [0, 30, 60, 90]
    if geometry == "disc":
        for (t, fx, fy, _, _), (_, rx, ry) in zip(rows, want.forces):
            print(f"t={t}: lbmo_forces ({fx:.17g}, {fy:.17g}) link_forces ({rx:.17g}, {ry:.17g}) diff ({abs(fx - rx):.2e}, {abs(fy - ry):.2e})")
        assert_forces_match([r[:3] for r in rows], want.forces, "lbmo_forces against link_forces")


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_no_slip_reference_is_the_oracle_bit_for_bit(geometry):
    """The loop every feature uses, its numpy boundary step included, with two no-slip walls named: f_current too, over 240 steps."""
    steps = 240
    ref, fcur = oracle_run(NX, NY, steps, 0, mask=mask_of(geometry), walls=(NOSLIP, NOSLIP), keep_f_current=True, **KW)
    o = Oracle(make_params(NX, NY, **KW))
    if geometry == "square":
        o.solid[:] = square(NX, NY)
        o.L.lbmo_initialise(o.h)
    assert o.run(steps) == -1 and ref.first_unstable == -1
    for name, got, want in (("f_current", fcur, o.f_current), ("f_next", ref.f_next, o.f_next), ("rho", ref.rho, o.rho),
                            ("ux", ref.ux, o.ux), ("uy", ref.uy, o.uy)):
        assert np.array_equal(got, want), name
    assert ref.solid_count == o.solid_count()
    o.close()


# ---- feature crosses: one feature, switched on in a way that must change nothing, under another -------------------------------------
def test_a_constant_schedule_under_walls_is_the_scaled_profile():
    c, walls = 0.7, (moving(0.05), FREESLIP)
    u = 0.1 * (np.arange(NY) + 1.0) / NY
    got = oracle_run(NX, NY, STEPS, OF, mask=square(NX, NY), u=u, walls=walls, schedule=([c], HOLD), **KW)
    want = oracle_run(NX, NY, STEPS, OF, mask=square(NX, NY), u=c * u, walls=walls, **KW)
    assert_same_run(got, want)
    away = oracle_run(NX, NY, STEPS, OF, mask=square(NX, NY), u=c * u, **KW)           # ... and the walls were active in both
    assert float(np.max(np.abs(want.f_next - away.f_next))) > 1e-3


def test_the_schedule_of_one_under_trt_is_no_schedule():
    trt = functools.partial(trt_collide, magic=3.0 / 16.0)
    got = oracle_run(NX, NY, STEPS, OF, collide=trt, schedule=([1.0], HOLD), **KW)
    want = oracle_run(NX, NY, STEPS, OF, collide=trt, **KW)
    assert_same_run(got, want)
    assert not np.array_equal(want.f_next, plain("disc").f_next)                      # ... and TRT was active in both
