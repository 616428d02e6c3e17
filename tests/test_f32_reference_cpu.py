"""The float32 reference of the fp32 kernels, checked without a GPU.

tests/numpy_oracle.py restates oracle/lbm_oracle.c in numpy for any element type; with dtype=np.float32 the reference loops
(tests/reference.py oracle_run, tests/ports_reference.py ports_run, tests/periodic_reference.py periodic_run) run on it, and
tests/test_gpu_f32_oracle.py holds the strict fp32 plans to the result bit for bit. Here: in float64 the restatement is the C oracle to
the bit, which pins the transcription everything float32 rests on; a float32 run stays float32 through every phase and is not a
float64 run cast at the end; and the float32 floor of every GPU case (the float32 reference against the float64 one) is positive and,
times four, below the bars the fp32 kernels were held to before (2e-5 on rho, 2e-4 on u)."""
import functools

import numpy as np
import pytest

from tests import f32_oracle_cases as oc
from tests import feature_cases as fc
from tests.helpers import golden_params, load_golden
from tests.mrt_reference import mrt_collide
from tests.numpy_oracle import NumpyOracle
from tests.periodic_reference import periodic_boundaries, periodic_run
from tests.ports_reference import PRESSURE, VELOCITY, port_of, ports_run
from tests.ports_reference import boundaries as ported_boundaries
from tests.reference import boundaries, open_run, oracle_run, snapshot

FIELDS = ("f_next", "rho", "ux", "uy")


def assert_same_runs(a, b, what):
    """Two (Run, f_current) pairs are one, bit for bit (equal_nan: a run that went unstable holds NaN in both)."""
    (ra, fa), (rb, fb) = a, b
    assert ra.first_unstable == rb.first_unstable and ra.solid_count == rb.solid_count, what
    for k in FIELDS:
        x, y = getattr(ra, k), getattr(rb, k)
        assert x.dtype == y.dtype == np.float64 and np.array_equal(x, y, equal_nan=True), "%s: %s differs" % (what, k)
    assert np.array_equal(fa, fb, equal_nan=True), "%s: f_current differs" % what
    assert len(ra.forces) == len(rb.forces) and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(ra.forces, rb.forces)), what
    assert np.array_equal(ra.solid, rb.solid)


def both_back_ends(loop, *args, **kw):
    return loop(*args, keep_f_current=True, **kw), loop(*args, keep_f_current=True, backend="numpy", **kw)


# ---- 1. in float64 the numpy restatement is the C oracle, bit for bit ------------------------------------------------------------------
def test_float64_equals_the_c_oracle_on_the_golden_parameters():
    p = golden_params(load_golden("g1_128x32_s10"))
    nx, ny = p.pop("nx"), p.pop("ny")
    a, b = both_back_ends(oracle_run, nx, ny, 12, 5, **p)
    assert a[0].first_unstable == -1 and len(a[0].forces) == 3
    assert_same_runs(a, b, "golden g1")


@pytest.mark.parametrize("case", fc.fp32_cases(), ids=fc.case_id)
def test_float64_equals_the_c_oracle_on_the_sweep_physics(case):
    a, b = both_back_ends(oracle_run, case.nx, case.ny, fc.steps_of(case), case.of, **fc.physics_kw(case))
    assert_same_runs(a, b, str(case))


def test_float64_equals_the_c_oracle_with_ports_periodic_y_and_mrt():
    kw = dict(walls=oc.WALLS, tau=0.6, inlet_velocity=0.05)
    assert_same_runs(*both_back_ends(ports_run, 65, 25, 23, 8, ports=((PRESSURE, 1.015), (VELOCITY, 0.03)), **kw), "ports")
    c = oc.CASES[oc.PERIODIC]
    a, b = both_back_ends(periodic_run, c.nx, c.ny, 24, 5, **c.ref_kw)
    assert a[0].solid[0, 40] and a[0].solid[-1, 40]                     # (the body across the seam)
    assert_same_runs(a, b, "periodic seam")
    mrt = functools.partial(mrt_collide, bulk_rate=1.0, magic=3.0 / 16.0)
    assert_same_runs(*both_back_ends(oracle_run, 130, 70, 23, 8, collide=mrt, **kw), "mrt")


def test_the_numpy_oracle_scans_ghost_and_solid_cells_for_stability():
    """lbmo_check_stability: a value beyond 1e5 anywhere in f_current, a ghost or a solid cell included, and 1e5 itself in the tail."""
    from oracle.oracle import Oracle, make_params
    c = Oracle(make_params(12, 7))
    for dtype in (np.float64, np.float32):
        o = NumpyOracle(make_params(12, 7), dtype)
        assert o.stable() and c.stable() and o.solid_count() == c.solid_count() == 1 and o.solid[3, 2]

        def verdict(idx, v):
            o.f_current[idx] = v
            c.f_current[idx] = v
            got = o.stable()
            assert got == c.stable(), (idx, v)
            o.f_current[idx] = 1.0
            c.f_current[idx] = 1.0
            return got
        for idx in ((0, 0, 0), (4, 3, 4), (3, 13, 4)):                  # a corner ghost, the solid cell, an E ghost column
            assert not verdict(idx, 2e5) and not verdict(idx, -2e5) and not verdict(idx, np.nan) and not verdict(idx, np.inf)
        assert o.f_current.size % 4 == 2
        assert verdict((0, 0, 0), 1e5)                                  # the vector part flags > 1e5 only,
        assert not verdict((8, 13, 8), 1e5)                             # the scalar tail |v| >= 1e5
    c.close()


# ---- 2. a float32 run is float32 throughout, and is not a float64 run cast at the end ---------------------------------------------------
@pytest.mark.parametrize("model", list(oc.MODELS))
def test_float32_stays_float32_through_every_phase(model):
    c = oc.CASES[oc.FAMILIES[model]]
    collide, walls = c.ref_kw["collide"], c.ref_kw["walls"]
    o, solid, u_at = open_run(66, 50, np.float32, None, None, every_row(50), (np.array([0.5, 1.0, 0.75]), 1), tau=c.ref_kw["tau"],
                              inlet_velocity=0.05)
    assert isinstance(o, NumpyOracle)

    def check(phase):
        for k in ("f_current",) + FIELDS:
            assert getattr(o, k).dtype == np.float32, (phase, k)
    check("initial state")
    for t in range(4):
        assert u_at(t).dtype == np.float32
        o.collide() if collide is None else collide(o, o.p.tau)
        check("collide")
        o.exchange_physical()
        check("exchange")
        o.set_ghost_row(0, o.edge_row(1))
        check("ghost row")
        o.stream()
        check("stream")
        boundaries(o, solid, walls, u_at(t))
        check("boundaries")
        ported_boundaries(o, solid, walls, u_at(t), (port_of((PRESSURE, 1.01), None), port_of((VELOCITY, 0.03), None)))
        check("ports")
        periodic_boundaries(o, solid, u_at(t), (port_of(VELOCITY, None), port_of((PRESSURE, 0.99), None)))
        check("periodic ports")
        assert o.stable()


def every_row(ny):
    from tests.helpers import every_row_differs
    return every_row_differs(ny, 0.05)


@pytest.mark.parametrize("name", [oc.FAMILIES["bgk"], oc.FAMILIES["forced"], "rows-schedule", "ports-pressure1.015-velocity0.03", oc.PERIODIC])
def test_float32_is_not_float64_cast_at_the_end(name):
    r32, r64 = oc.reference(name, "f32"), oc.reference(name, "f64")
    for k in FIELDS:
        assert getattr(r32, k).dtype == np.float32 and getattr(r64, k).dtype == np.float64
    assert r32.first_unstable == r64.first_unstable == -1 and r32.solid_count == r64.solid_count
    cast = r64.f_next.astype(np.float32)
    differ = int(np.sum(cast != r32.f_next))
    assert differ > r32.f_next.size // 10, differ                       # its own rounding history: most values, not a few
    assert all(isinstance(v, float) for row in r32.forces for v in row[1:])


# ---- 3. the snapshot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [oc.FAMILIES["bgk"], oc.FAMILIES["forced"], "edges-65x25-0", "smallest-2x2-1", oc.PERIODIC])
def test_snapshot_is_the_oracles_macros_up_to_rounding_and_equal_where_the_oracle_records_them(name):
    for precision, bar_rho, bar_u in (("f64", 1e-14, 1e-10), ("f32", 2e-6, 2e-6)):
        ref = oc.reference(name, precision)
        rho, ux, uy = snapshot(ref)
        assert rho.dtype == ux.dtype == uy.dtype == ref.rho.dtype
        for x in (0, ref.solid.shape[1] - 1):                           # the port columns: what `boundaries` recorded
            assert np.array_equal(rho[:, x], ref.rho[:, x]) and np.array_equal(ux[:, x], ref.ux[:, x]) and np.all(uy[:, x] == 0.0)
        s = ref.solid
        assert np.all(rho[s] == 1.0) and np.all(ux[s] == 0.0) and np.all(uy[s] == 0.0)
        assert float(np.max(np.abs(rho - ref.rho))) <= bar_rho
        assert max(float(np.max(np.abs(ux - ref.ux))), float(np.max(np.abs(uy - ref.uy)))) <= bar_u
        if ref.solid.shape[1] > 2:
            assert not np.array_equal(rho, ref.rho)                     # (moments of other populations: equal sums up to rounding only)


# ---- 4. the float32 floor of every GPU case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CASES))
def test_floor_of_every_gpu_case_is_positive_and_four_floors_are_below_the_earlier_bars(name):
    r32, r64 = oc.reference(name, "f32"), oc.reference(name, "f64")
    assert r32.first_unstable == r64.first_unstable == -1
    assert [r[0] for r in r32.forces] == [r[0] for r in r64.forces]
    floor_f, floor_rho, floor_u = oc.floors(name)
    print("floor %s: f %.3g rho %.3g u %.3g" % (name, floor_f, floor_rho, floor_u))
    assert floor_f > 0.0 and floor_rho > 0.0 and floor_u > 0.0
    assert 4.0 * floor_rho < 2e-5 and 4.0 * floor_u < 2e-4, (floor_rho, floor_u)


def test_sweep_references_in_float32():
    """feature_cases.reference32_of: the physics of reference_of in float32 (one stable case and its floor)."""
    case = next(c for c in fc.fp32_cases() if fc.reference_of(c).first_unstable == -1 and fc.steps_of(c) > 20 and c.nx * c.ny > 2000)
    r32, r64 = fc.reference32_of(case), fc.reference_of(case)
    assert r32.f_next.dtype == np.float32 and r32.first_unstable == -1 and r32.solid_count == r64.solid_count
    floor = oc.floors_of_runs(r32, r64)
    assert all(0.0 < v < 1e-3 for v in floor), floor
