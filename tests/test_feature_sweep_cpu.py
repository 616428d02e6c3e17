"""The guard of the feature sweep (tests/feature_cases.py, tests/test_gpu_feature_sweep.py), without a GPU: the generator is
deterministic, draws only what the library accepts and covers what it claims to; the references are stable, so that a case checks fields
and not one integer; every feature changes the reference it is part of; and the lean-tile cases do have lean tiles."""
import collections
import os
import re

import numpy as np
import pytest

from oracle.oracle import Oracle, make_params
from tests import feature_cases as fc
from tests.helpers import PKG, PLANS, ROOT, deep_shapes
from tests.reference import FREESLIP, NOSLIP, oracle_run

ALL = fc.fp64_cases() + fc.fp32_cases()


# ---- the generator -------------------------------------------------------------------------------------------------------------------
def test_the_generator_is_deterministic():
    assert fc.fp64_cases() == fc.fp64_cases() and fc.fp32_cases() == fc.fp32_cases()
    assert len(fc.fp64_cases()) == 120 and len(fc.fp32_cases()) == 40
    assert [c.k for c in fc.fp64_cases()] == list(range(120)) and len(set(fc.case_id(c) for c in ALL)) == len(ALL)
    for c in ALL:
        hash(c)                                     # a case is its own cache key
        assert eval(repr(c), {"Case": fc.Case}) == c, c          # ... and prints completely


def model_rows():
    """{model: (tall, park)} as csrc/lbm_plan.hpp collision_models grants the tall fp32 (deep 8) and the tall fp64 (deep 10 / 11) regions."""
    text = open(os.path.join(ROOT, PKG, "csrc", "lbm_plan.hpp")).read()
    consts = dict(re.findall(r"\b(PARK_\w+) = (true|false)", text))
    rows = re.findall(r"\{(AR_STRICT\w*), \"[^\"]*\", (true|false), (\w+),", text)
    assert [r[0] for r in rows] == ["AR_STRICT", "AR_STRICT_LES", "AR_STRICT_TRT", "AR_STRICT_FORCED"], rows
    return {m: (tall == "true", consts.get(park, park) == "true") for m, (_, tall, park) in zip(fc.MODELS, rows)}


def test_every_case_is_one_the_library_accepts():
    rows = model_rows()
    assert rows["bgk"] == (True, True)
    for c in ALL:
        assert 2 <= c.nx <= 420 and 2 <= c.ny <= 150 and 1 <= fc.steps_of(c) <= 150 and 1 <= c.of <= 45, c
        assert 1 <= len(c.calls) <= 3 and min(c.calls) >= 1 and sum(fc.issued_calls(c)) == fc.steps_of(c), c
        assert not c.trailing_pair or fc.issued_calls(c)[-1] == 1, c                    # the state is read after a single step
        assert (c.param is None) == (c.model == "bgk"), c                                  # one model, never two
        opts = fc.options_of(c)
        deep = opts.get("deep", 0)
        assert opts["tune"] == 0 and (c.plan in PLANS or c.plan in fc.PINNED), c
        tall, park = rows[c.model]
        if deep == 8:                                # (set_option refuses it on fp64; set_smagorinsky / set_trt / set_forcing refuse it)
            assert c.precision == "f32" and tall, c
        if deep in (10, 11):                         # (lbm_initialise: contracted arithmetic on whole domains only; set_option: fp64 only)
            assert c.precision == "f64" and park and opts["arith"] == 1, c
        if c.strips > 1:                             # (lbm_group_link: a strip with neighbours needs at least twelve rows)
            assert c.ny >= 40 and c.strips <= min(4, c.ny // 12) and deep not in (8, 10, 11), c
            assert opts["layout"] == 1 and opts["alternate"] == 0 and 0 <= opts["overlap"] <= 2 and 0 <= opts["deep_halo"] <= 2, c
        for w in c.walls:
            assert w in (NOSLIP, FREESLIP) or (w[0] == "moving" and abs(w[1]) <= 0.06), c
        assert 0.01 <= c.u <= 0.08 and (0.52 <= c.tau <= 0.6 if c.model == "les" else 0.56 <= c.tau <= 1.1), c
        if c.model == "trt":
            assert c.param in fc.MAGICS and c.tau > 0.5, c
        if c.model == "forced":
            assert max(abs(c.param[0]), abs(c.param[1])) <= 5e-5 and c.param != (0.0, 0.0), c
        if c.schedule:
            s, _ = fc.schedule_of(c)
            assert 1 <= len(s) <= 40 and s.min() >= 0.2 and s.max() <= 1.0, c
        if c.ckpt_plan:                              # a checkpoint is handed to another family in the same arithmetic mode, never in a group
            assert c.precision == "f64" and c.strips == 1 and len(c.calls) > 1 and c.ckpt_plan in PLANS, c
            assert fc.contracted(c.ckpt_plan) == fc.contracted(c.plan) and fc.family(c.ckpt_plan) != fc.family(c.plan), c


def test_the_cases_cover_what_they_claim():
    for cases, families in ((fc.fp64_cases(), ["site", "pair", "fuse3", "fuse4", "deep", "col", "park"]), (fc.fp32_cases(), ["tall", "col", "site"])):
        def count(key):
            return collections.Counter(v for c in cases for v in key(c))
        for what, key, values in (
                ("model", lambda c: [c.model], fc.MODELS),
                ("wall", lambda c: [w if isinstance(w, str) else w[0] for w in c.walls], [NOSLIP, FREESLIP, "moving"]),
                ("geometry", lambda c: [c.geometry], fc.GEOMETRIES),
                ("schedule", lambda c: [c.schedule[1] if c.schedule else "none"], ["none", "hold", "repeat"]),
                ("profile", lambda c: [c.profile], [0, 1]),
                ("family", lambda c: [fc.family(c.plan)], families),
                ("arith", lambda c: [fc.contracted(c.plan)], [0, 1]),
                ("strips", lambda c: [c.strips], [1, 2, 3, 4])):
            n = count(key)
            assert all(n[v] >= 3 for v in values), (cases[0].precision, what, dict(n))
        n = collections.Counter(c.model for c in cases)
        assert len(set(n.values())) == 1, n                                           # the four models equally
    # no model but BGK ever ran on a grid narrower than a tile or lower than a region, or on strips: each does here, more than once
    for m in fc.MODELS[1:]:
        assert sum(1 for c in fc.fp64_cases() if c.model == m and (c.nx < 52 or c.ny < 20)) >= 2, m
        assert sum(1 for c in fc.fp64_cases() if c.model == m and c.strips > 1) >= 2, m
    single = [c for c in fc.fp64_cases() if c.strips == 1]
    assert len(single) / 4 <= sum(1 for c in single if c.ckpt_plan) <= len(single) / 2          # roughly a third through a checkpoint


# ---- the references ------------------------------------------------------------------------------------------------------------------
def test_few_references_go_unstable():
    """An unstable case checks one integer: at most a tenth of them may be."""
    cases = fc.fp64_cases()
    bad = [(c.k, fc.reference_of(c).first_unstable) for c in cases if fc.reference_of(c).first_unstable != -1]
    print("unstable references: %d of %d %s" % (len(bad), len(cases), bad))
    assert len(bad) <= len(cases) // 10, bad
    for c in cases:
        ref = fc.reference_of(c)
        if ref.first_unstable == -1:
            assert np.all(np.isfinite(ref.f_next)) and [r[0] for r in ref.forces] == list(range(0, fc.steps_of(c), c.of)), c
    for model in fc.LEAN_MODELS:
        ref = fc.lean_reference(model)
        assert ref.first_unstable == -1 and np.all(np.isfinite(ref.f_next)) and ref.solid_count > 0, model


FEATURES = {
    # feature -> (which cases have it, the reference's keywords with it switched off)
    "les": (lambda c: c.model == "les", lambda c: dict(collide=None)),
    "trt": (lambda c: c.model == "trt", lambda c: dict(collide=None)),
    "forcing": (lambda c: c.model == "forced", lambda c: dict(collide=None)),
    "walls": (lambda c: c.walls != (NOSLIP, NOSLIP), lambda c: dict(walls=NOSLIP)),
    "schedule": (lambda c: c.schedule is not None, lambda c: dict(schedule=None)),
    "profile": (lambda c: bool(c.profile), lambda c: dict(u=None)),
    "mask": (lambda c: c.geometry in ("random", "boundaries"), lambda c: dict(mask=np.zeros((c.ny, c.nx), np.uint8))),
}


@pytest.mark.parametrize("feature", list(FEATURES))
def test_every_feature_changes_its_reference(feature):
    """The case with the most iterations among those with the feature on a lattice of at least 24x24: without the feature the reference is
    another one, so no case can pass with the feature doing nothing."""
    has, off = FEATURES[feature]
    c = max((c for c in fc.fp64_cases() if has(c) and c.nx >= 24 and c.ny >= 24 and fc.steps_of(c) >= 20), key=fc.steps_of)
    ref = fc.reference_of(c)
    other = oracle_run(c.nx, c.ny, fc.steps_of(c), c.of, **fc.physics_kw(c, **off(c)))
    assert ref.first_unstable == -1 and other.first_unstable == -1, c
    away = float(np.max(np.abs(ref.f_next - other.f_next)))
    assert away > 1e-6, (feature, away, c)


@pytest.mark.parametrize("model", [m for m in fc.LEAN_MODELS if m != "bgk"])
def test_the_lean_cases_feel_their_model_and_walls(model):
    ref, bgk, plain = fc.lean_reference(model), fc.lean_reference("bgk"), fc.lean_reference(model, (NOSLIP, NOSLIP))
    # (LES at tau 0.51 against BGK at 0.55: another tau as well as another operator)
    assert float(np.max(np.abs(ref.f_next - bgk.f_next))) > 1e-6 and float(np.max(np.abs(ref.f_next - plain.f_next))) > 1e-6


# ---- the lean tiles ------------------------------------------------------------------------------------------------------------------
def region_height(precision, strict, tall):
    """Rows per thread * waves of the register kernel's regions as the library's table has them (csrc/lbm_plan.hpp region_kinds): 24 strict
    fp64, 32 contracted fp64, 40 parked, 32 fp32, 48 tall fp32. `tall`: the kind of deep 8 (fp32) / deep 10 (fp64), else that of deep 7."""
    return deep_shapes()[(7 if not tall else 10 if precision == "f64" else 8), precision, int(not strict)].h


def tile_shape(plan, precision):
    """(OW, OH, HW) of the fused kernel the plan pins: its output tile and the rings its first level reaches beyond it, HW = D - 1.
    The register kernel (k_stepc_col): OW = 64 - 2 HW, OH = region height - 2 HW. The LDS tile families hand the same TileFrame their
    tile: 64x16 (32x32 at eight iterations) for k_stepd_tile (deep_shapes, csrc/lbm_plan.hpp), 64 x pair_ty (64x8 at four) for
    k_step3_tile / k_step4_tile. None: one or two iterations per launch (k_step_site, k_step2_tile), which have no LEAN path."""
    o = fc.plan_options(plan)
    deep, strict = o.get("deep", 0), not o.get("arith", 0)
    if deep:
        row = deep_shapes()[deep, precision, int(not strict)]
        hw = row.depth - 1
        return (row.w - 2 * hw, row.h - 2 * hw, hw) if row.family == "registers" else (row.w, row.h, hw)
    fuse = o.get("fuse", 1)
    return (64, 8 if fuse == 4 else o["pair_ty"], fuse - 1) if fuse in (3, 4) and not o.get("pair") else None


def count_tiles(nx, ny, shape, solid):
    """(lean, general) tiles of a whole-domain launch: TileFrame's inequality (csrc/lbm_kernels.hpp) on the tiles at (bx OW, by OH), with
    the conservative near-solid condition: no solid cell within HW + 8 cells of the output tile (the mask query rounds outward to 8x8
    blocks, the disc query to its bounding box)."""
    ow, oh, hw = shape
    lean = general = 0
    for y0 in range(0, ny, oh):
        for x0 in range(0, nx, ow):
            inside = x0 >= hw + 1 and x0 + ow + hw <= nx - 1 and y0 >= hw + 1 and y0 + oh + hw <= ny - 1 and y0 + oh <= ny
            r = hw + 8
            far = not solid[max(0, y0 - r):y0 + oh + r, max(0, x0 - r):x0 + ow + r].any()
            lean, general = lean + (inside and far), general + (not (inside and far))
    return lean, general


def disc(nx, ny, **kw):
    o = Oracle(make_params(nx, ny, **kw))
    solid = o.solid.astype(bool).copy()
    o.close()
    return solid


def test_region_heights():
    assert [region_height(*a) for a in (("f64", True, False), ("f64", False, False), ("f64", False, True), ("f32", True, False),
                                        ("f32", False, False), ("f32", True, True), ("f32", False, True))] == [24, 32, 40, 32, 32, 48, 48]
    assert tile_shape("fast-rowil-col6", "f64") == (54, 22, 5) and tile_shape("fast-planar-col5", "f64") == (56, 24, 4)
    assert tile_shape("rowil-col5-nt", "f64") == (56, 16, 4) and tile_shape("park11", "f64") == (52, 28, 6)
    assert tile_shape("tall-f32", "f32") == (52, 36, 6) and tile_shape("rowil-site-nt", "f64") is None


def test_the_lean_cases_have_lean_and_general_tiles():
    solid = disc(fc.LEAN_NX, fc.LEAN_NY)
    assert solid.any()
    for plan in fc.LEAN_PLANS:
        shape = tile_shape(plan, "f64")
        if shape is not None:
            lean, general = count_tiles(fc.LEAN_NX, fc.LEAN_NY, shape, solid)
            assert lean >= 1 and general >= 1, (plan, shape, lean, general)
    assert sum(1 for p in fc.LEAN_PLANS if fc.family(p) in ("col", "park")) == 8        # the register plans: each was counted above
    solid = disc(fc.LEAN_NX, fc.LEAN_NY_F32)
    for _, plan in fc.LEAN_PLANS_F32:
        lean, general = count_tiles(fc.LEAN_NX, fc.LEAN_NY_F32, tile_shape(plan, "f32"), solid)
        assert lean >= 1 and general >= 1, (plan, lean, general)


def test_the_feature_suites_lattice_has_no_lean_tile_on_the_contracted_register_plans():
    """160x48, the lattice of the per-feature tests: the two contracted register plans they hold to the reference (one of them the
    plan the benchmark times) have no lean tile there even without an obstacle: band 1 ends at row 22 + 22 + 5 = 49 (six iterations) and
    24 + 24 + 4 = 52 (five), above row 47. The strict 64x24 shape and seven iterations do get one."""
    empty = np.zeros((48, 160), bool)
    for plan in ("fast-rowil-col6", "fast-planar-col5"):
        assert count_tiles(160, 48, tile_shape(plan, "f64"), empty)[0] == 0, plan
    for plan in ("rowil-col5-nt", "planar-col6-alt", "rowil-col7-alt", "fast-rowil-col7"):
        assert count_tiles(160, 48, tile_shape(plan, "f64"), empty)[0] >= 1, plan
