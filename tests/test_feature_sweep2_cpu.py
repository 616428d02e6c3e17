"""The guard of the second feature sweep (tests/feature_cases2.py, tests/test_gpu_feature_sweep2.py), without a GPU: the first
generation's cases have not moved; the new generator is deterministic, draws only what the library accepts and covers what it claims to;
few references go unstable; periodic y, the ports and MRT each change the reference they are part of; the reference's seam is checked
against a loop over cells; and without periodicity and ports the reference loop is oracle_run to the bit."""
import collections
import hashlib
import os
import re

import numpy as np
import pytest

from tests import feature_cases as fc
from tests import feature_cases2 as f2
from tests.helpers import PKG, ROOT
from tests.periodic_reference import periodic_boundaries, periodic_link_forces, periodic_run
from tests.ports_reference import DEFAULT_PORTS, PRESSURE, VELOCITY, port_rule
from tests.reference import CX, CY, FREESLIP, NOSLIP, OPP, open_run, oracle_run
from tests.test_feature_sweep_cpu import FEATURES as FEATURES1, model_rows
from tests.test_gpu_periodic import PERIODIC_PLANS

F64, F32 = f2.fp64_cases(), f2.fp32_cases()
ALL = F64 + F32


# ---- the first generation stays where it is -------------------------------------------------------------------------------------------
def test_the_first_generation_has_not_moved():
    """SHA-256 of the printed first-generation cases, taken before this module existed: "they never change" is their contract."""
    digest = hashlib.sha256(repr(fc.fp64_cases() + fc.fp32_cases()).encode()).hexdigest()
    assert digest == "68f04c34031e386d688a8fa530692612b2abc954041a7a35e576fe4678dc7071", digest


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    assert f2.fp64_cases() == F64 and f2.fp32_cases() == F32
    assert len(F64) == 96 and len(F32) == 32
    assert [c.k for c in F64] == list(range(96)) and len(set(f2.case_id(c) for c in ALL)) == len(ALL)
    assert f2.Case2._fields == fc.Case._fields + ("periodic", "ports", "bounds")
    for c in ALL:
        hash(c)                                     # a case is its own cache key
        assert eval(repr(c), {"Case2": f2.Case2}) == c, c          # ... and prints completely
    assert hashlib.sha256(repr(ALL).encode()).hexdigest() == "e1fef67cf437ea60856fd5baf0d71b5627793985bebe8ef94588365c24724d72"          # (and they, too, never change)


def mrt_row():
    """(tall, park) of the designated-initialiser MRT row of csrc/lbm_plan.hpp collision_models (model_rows() of
    tests/test_feature_sweep_cpu.py parses the four positional rows)."""
    text = open(os.path.join(ROOT, PKG, "csrc", "lbm_plan.hpp")).read()
    consts = dict(re.findall(r"\b(PARK_\w+) = (true|false)", text))
    rows = re.findall(r"\{\.base = (AR_STRICT\w*),[^}]*?\.tall = (true|false),[^}]*?\.park = (\w+),", text)
    assert [r[0] for r in rows] == ["AR_STRICT_MRT"], rows
    return rows[0][1] == "true", consts.get(rows[0][2], rows[0][2]) == "true"


def all_model_rows():
    rows = dict(model_rows(), mrt=mrt_row())
    assert list(rows) == list(f2.MODELS)
    return rows


def test_every_case_is_one_the_library_accepts():
    rows = all_model_rows()
    assert rows["bgk"] == (True, True) and rows["mrt"] == (False, False)
    for cases in (F64, F32):
        assert [c.model for c in cases] == [f2.ROTATION[c.k % 6] for c in cases]                # the models in rotation
        assert sum(c.periodic for c in cases) * 2 == len(cases)                                  # half the cases are periodic
        assert sum(1 for c in cases if c.model == "mrt") in (len(cases) // 3, (len(cases) + 2) // 3)
    for c in ALL:
        assert 2 <= c.nx <= 260 and 2 <= c.ny <= 150 and 1 <= f2.steps_of(c) <= 100 and 1 <= c.of <= 45, c
        assert 1 <= len(c.calls) <= 3 and min(c.calls) >= 1 and sum(f2.issued_calls(c)) == f2.steps_of(c), c
        assert not c.trailing_pair or f2.issued_calls(c)[-1] == 1, c
        assert c.model in f2.MODELS and (c.param is None) == (c.model == "bgk"), c                # one model, never two
        assert sum(k in f2.context_kw(c) for k in ("smagorinsky", "trt_magic", "forcing", "mrt")) == (c.model != "bgk"), c
        opts = f2.options_of(c)
        deep = opts.get("deep", 0)
        tall, park = rows[c.model]
        assert opts["tune"] == 0, c
        if deep == 8:
            assert c.precision == "f32" and tall, c
        if deep in (10, 11):
            assert c.precision == "f64" and park and opts["arith"] == 1 and not c.periodic, c
        if c.model == "mrt":                                  # (collision_models: no tall fp32 and no tall fp64 regions)
            assert deep not in (8, 10, 11), c
        # periodic: both walls no-slip, at least twelve rows, row-interleaved, no row-range launches, no whole-domain-only shape
        if c.periodic:
            assert c.walls == (NOSLIP, NOSLIP) and c.ny >= 12 and opts["layout"] == 1 and not opts.get("split") and deep not in (10, 11), c
            assert c.plan in PERIODIC_PLANS or (c.plan in f2.PERIODIC_TALL and c.precision == "f32" and c.model == "bgk"), c
            assert c.geometry in f2.GEOMETRIES2, c
        else:
            assert c.plan in fc.PLAN_KEYS or c.plan in fc.PINNED, c
            assert c.geometry in fc.GEOMETRIES and c.bounds != ((0, c.ny),), c
            for w in c.walls:
                assert w in (NOSLIP, FREESLIP) or (w[0] == "moving" and abs(w[1]) <= 0.06), c
        # strips: two to four (a ring of one), each of at least twelve rows, tiling the lattice; peer transport on device 0
        if f2.grouped(c):
            b = f2.bounds_of(c)
            assert c.ny >= (24 if c.periodic else 40) and 1 <= len(b) <= 4 and (len(b) > 1 or c.periodic), c
            assert b[0][0] == 0 and all(a[0] + a[1] == n[0] for a, n in zip(b, b[1:])) and b[-1][0] + b[-1][1] == c.ny, c
            assert min(r for _, r in b) >= 12 and len(b) == (c.strips if c.bounds is None else len(c.bounds)), c
            if c.bounds is not None and len(b) > 1:
                assert 12 in [r for _, r in b], c
            assert deep not in (8, 10, 11) and c.ckpt_plan is None, c
            assert opts["layout"] == 1 and opts["alternate"] == 0 and 0 <= opts["overlap"] <= 2 and 0 <= opts["deep_halo"] <= 2, c
        else:
            assert c.strips == 1 and c.strip_opts is None, c
        # the ports at the magnitudes of tests/test_gpu_ports.py; a west pressure port takes neither a profile nor a schedule
        west, east = c.ports
        assert west == VELOCITY or (west[0] == PRESSURE and 1.0 <= west[1] <= 1.015), c
        assert (east[0] == PRESSURE and 0.985 <= east[1] <= 1.0) or (east[0] == VELOCITY and 0.0 <= east[1] <= 0.03), c
        if west != VELOCITY:
            assert not c.profile and c.schedule is None, c
        assert 0.01 <= c.u <= 0.08 and (0.52 <= c.tau <= 0.6 if c.model == "les" else 0.56 <= c.tau <= 1.1), c
        if c.model == "trt":
            assert c.param in fc.MAGICS, c
        if c.model == "mrt":
            assert 0.6 <= c.param[0] <= 1.9 and c.param[1] in fc.MAGICS and c.tau > 0.5, c
        if c.model == "forced":
            assert max(abs(c.param[0]), abs(c.param[1])) <= 5e-5 and c.param != (0.0, 0.0), c
        if c.schedule:
            s, _ = f2.schedule_of(c)
            assert 1 <= len(s) <= 40 and s.min() >= 0.2 and s.max() <= 1.0, c
        if c.ckpt_plan:             # handed to another family (periodic: another strip plan) in the same arithmetic mode, never in a group
            assert c.precision == "f64" and len(c.calls) > 1, c
            assert c.ckpt_plan in (PERIODIC_PLANS if c.periodic else fc.HANDOVER[f2.contracted(c.plan, 0)]), c
            assert f2.contracted(c.ckpt_plan, c.periodic) == f2.contracted(c.plan, c.periodic), c
            assert f2.family(c.ckpt_plan, c.periodic) != f2.family(c.plan, c.periodic), c
            assert rows[c.model][1] or f2.plan_options(c.ckpt_plan, c.periodic).get("deep", 0) not in (10, 11), c


def nstrips(c):
    return len(f2.bounds_of(c)) if f2.grouped(c) else 1


def unequal_with_twelve(c):
    return c.bounds is not None and len(c.bounds) > 1 and 12 in [r for _, r in c.bounds] and len(set(r for _, r in c.bounds)) > 1


COVERAGE = [
    # (what, the values a case counts for, the values that must be hit)
    ("model", lambda c: [c.model], f2.MODELS),
    ("west port", lambda c: ["velocity" if c.ports[0] == VELOCITY else "pressure"], ["velocity", "pressure"]),
    ("east port", lambda c: [c.ports[1][0]], ["velocity", "pressure"]),
    ("periodic", lambda c: [c.periodic], [0, 1]),
    ("arith", lambda c: [f2.contracted(c.plan, c.periodic)], [0, 1]),
    ("strips", lambda c: [nstrips(c)], [1, 2, 3, 4]),
    ("unequal bounds with a twelve-row strip", lambda c: [unequal_with_twelve(c)], [True]),
    ("ring of one", lambda c: [c.bounds == ((0, c.ny),)], [True]),
    ("periodic ny < 16", lambda c: [c.periodic and c.ny < 16], [True]),
    ("periodic ny in 16..23", lambda c: [c.periodic and 16 <= c.ny <= 23], [True]),
    ("periodic nx < 52", lambda c: [c.periodic and c.nx < 52], [True]),
    ("periodic nx in 63..65", lambda c: [c.periodic and c.nx in (63, 64, 65)], [True]),
    ("seam geometry", lambda c: [c.geometry == "seam"], [True]),
    ("MRT on a small lattice", lambda c: [c.model == "mrt" and (c.nx < 52 or c.ny < 20)], [True]),
    ("MRT on strips", lambda c: [c.model == "mrt" and nstrips(c) > 1], [True]),
    ("MRT under periodic y", lambda c: [c.model == "mrt" and bool(c.periodic)], [True]),
    ("MRT under other ports", lambda c: [c.model == "mrt" and c.ports != DEFAULT_PORTS], [True]),
    ("ports on strips", lambda c: [c.ports != DEFAULT_PORTS and nstrips(c) > 1], [True]),
    ("periodic on strips", lambda c: [bool(c.periodic) and nstrips(c) > 1], [True]),
]


def coverage_problems(cases, least, families):
    out = []
    table = COVERAGE + [("family under periodic y", lambda c: [f2.family(c.plan, 1)] if c.periodic else [], families)]
    for what, key, values in table:
        n = collections.Counter(v for c in cases for v in key(c))
        out += ["%s %r: %d" % (what, v, n[v]) for v in values if n[v] < least]
    return out


def test_the_cases_cover_what_they_claim():
    assert not coverage_problems(F64, 3, ["site", "pair", "fuse3", "deep", "col"])
    assert not coverage_problems(F32, 2, ["site", "pair", "fuse3", "deep", "col", "tall"])
    single = [c for c in F64 if not f2.grouped(c)]
    assert len(single) / 4 <= sum(1 for c in single if c.ckpt_plan) <= len(single) / 2
    assert sum(1 for c in single if c.ckpt_plan and c.periodic) >= 3 and sum(1 for c in single if c.ckpt_plan and not c.periodic) >= 3


# ---- the references ------------------------------------------------------------------------------------------------------------------
def test_few_references_go_unstable():
    """An unstable case checks one integer: at most a tenth of them may be."""
    bad = [(c.k, f2.reference_of(c).first_unstable) for c in F64 if f2.reference_of(c).first_unstable != -1]
    print("unstable references: %d of %d %s" % (len(bad), len(F64), bad))
    assert len(bad) <= len(F64) // 10, bad
    for c in F64:
        ref = f2.reference_of(c)
        if ref.first_unstable == -1:
            assert np.all(np.isfinite(ref.f_next)) and [r[0] for r in ref.forces] == list(range(0, f2.steps_of(c), c.of)), c
    for nx, ny, variant in f2.SMALLEST_CASES:
        ref = f2.smallest_reference(nx, ny, variant)
        assert ref.first_unstable == -1 and np.all(np.isfinite(ref.f_next)) and ref.solid_count > 0, (nx, ny, variant)
        assert [r[0] for r in ref.forces] == [0, 3, 6, 9, 12], (nx, ny, variant)


FEATURES = dict(FEATURES1)
FEATURES.update({
    "mrt": (lambda c: c.model == "mrt", lambda c: dict(collide=None)),
    "ports": (lambda c: c.ports != DEFAULT_PORTS, lambda c: dict(ports=DEFAULT_PORTS)),
    "periodic": (lambda c: bool(c.periodic), lambda c: dict(periodic=False)),
})
FEATURES["mask"] = (lambda c: c.geometry in ("random", "boundaries", "seam"), FEATURES1["mask"][1])


@pytest.mark.parametrize("feature", list(FEATURES))
def test_every_feature_changes_its_reference(feature):
    """The case with the most iterations among those with the feature on a lattice of at least 24x24: without the feature the reference is
    another one, so no case can pass with the feature doing nothing."""
    has, off = FEATURES[feature]
    c = max((c for c in F64 if has(c) and c.nx >= 24 and c.ny >= 24 and f2.steps_of(c) >= 20 and f2.reference_of(c).first_unstable == -1),
            key=f2.steps_of)
    ref = f2.reference_of(c)
    other = periodic_run(c.nx, c.ny, f2.steps_of(c), c.of, **f2.physics_kw(c, **off(c)))
    assert other.first_unstable == -1, c
    away = float(np.max(np.abs(ref.f_next - other.f_next)))
    assert away > 1e-6, (feature, away, c)


def test_the_seam_cuts_the_seam_block():
    cut = [c for c in F64 if c.periodic and c.geometry == "seam" and f2.mask_of(c)[0].any() and f2.mask_of(c)[c.ny - 1].any()]
    assert len(cut) >= 3, len(cut)
    for nx, ny in f2.SMALLEST:
        m = f2.seam_block(nx, ny)
        assert m[0].any() and m[ny - 1].any() and m[:, 0].any() and m[:, nx - 1].any() and not m.all(), (nx, ny)
        u = f2.smallest_inputs(nx, ny, "plain")[0]["inlet_profile"]
        assert len(set(u.tolist())) == ny


def test_without_periodicity_and_ports_the_loop_is_oracle_run():
    cases = [c for c in F64 if not c.periodic and c.ports == DEFAULT_PORTS and f2.reference_of(c).first_unstable == -1][:3]
    assert len(cases) == 3
    for c in cases:
        kw = f2.physics_kw(c)
        del kw["periodic"], kw["ports"]
        want, got = oracle_run(c.nx, c.ny, f2.steps_of(c), c.of, **kw), f2.reference_of(c)
        assert np.array_equal(got.f_next, want.f_next) and got.forces == want.forces and got.solid_count == want.solid_count, c
        for a, b in zip((got.rho, got.ux, got.uy), (want.rho, want.ux, want.uy)):
            assert np.array_equal(a, b), c


# ---- the reference's seam against a loop over cells ----------------------------------------------------------------------------------
def test_the_references_seam_against_a_loop_over_cells():
    nx, ny = 3, 12
    mask = np.zeros((ny, nx), np.uint8)
    mask[0, 1] = mask[ny - 1, 1] = mask[ny - 1, 0] = mask[5, 2] = 1          # a body across the seam, a cell in each port column
    rng = np.random.default_rng(3)
    f = rng.uniform(0.01, 0.4, (ny + 2, nx + 2, 9))
    solid = mask.astype(bool)
    # link forces: every fluid cell, every direction, the neighbour's row taken mod ny, its column inside the domain
    fx = fy = 0.0
    links = 0
    for y in range(ny):
        for x in range(nx):
            for i in range(1, 9):
                xn, yn = x + CX[i], (y + CY[i]) % ny
                if not solid[y, x] and 0 <= xn < nx and solid[yn, xn]:
                    fx += 2.0 * CX[i] * f[y + 1, x + 1, i]
                    fy += 2.0 * CY[i] * f[y + 1, x + 1, i]
                    links += (y + CY[i]) != yn
    got = periodic_link_forces(f, solid)
    assert links >= 4 and abs(got[0] - fx) <= 1e-14 and abs(got[1] - fy) <= 1e-14, (got, fx, fy, links)
    # boundaries: no wall rule on row 0 or ny - 1; the port rules on the fluid cells of columns 0 and nx - 1; solid cells turned round
    ports = ((PRESSURE, 1.01), (VELOCITY, 0.02))
    o, s, u_at = open_run(nx, ny, np.float64, "numpy", mask, None, None, tau=0.6, inlet_velocity=0.05)
    assert np.array_equal(s, solid)
    o.f_current[:] = f
    before = f.copy()
    periodic_boundaries(o, solid, u_at(0), ports)
    for y in range(ny):
        for x in range(nx):
            cell = before[y + 1, x + 1].copy()
            if solid[y, x]:
                cell = cell[OPP]
            elif x in (0, nx - 1):
                one = cell[None, :].copy()
                port_rule(one, int(x == nx - 1), *ports[int(x == nx - 1)])
                cell = one[0]
            assert np.array_equal(o.f_current[y + 1, x + 1], cell), (x, y)
    assert np.array_equal(o.f_current[0], before[0]) and np.array_equal(o.f_current[ny + 1], before[ny + 1])        # (ghost rows: not its business)
    o.close()
