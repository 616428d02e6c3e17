"""Seeded cases of the feature sweep (test infrastructure; tests/test_gpu_feature_sweep.py runs them on the GPU,
tests/test_feature_sweep_cpu.py checks the generator and the references without one).

A case crosses what the per-feature tests hold to the reference at one friendly lattice each: a collision model (BGK, Smagorinsky
LES, TRT, BGK under a driving force: never two, the library refuses that), a geometry (the analytic disc, a random mask, a mask that
touches all four boundaries, an all-fluid mask), an inlet (uniform or a value per row, with or without a schedule table), the kind of
each wall, a sequence of step() calls, a plan of every kernel family, and (where the lattice is tall enough) a group of strips; on
ragged grids from 2x2 to 420x150 whose fixed sizes are the tile and region pitches +-1 of the register kernel's 64x24, 64x32 and 64x40
shapes at five, six and seven iterations per launch.

The generator is seeded and appends its cases in a fixed order: they never change. A case is a named tuple of numbers, strings and
tuples, so that it prints completely in a failure message and is its own cache key; the arrays it stands for (mask, inlet profile,
schedule table) are rebuilt from it by the functions below."""
import collections
import functools

import numpy as np

from tests.forcing_reference import guo_collide
from tests.helpers import PLANS, TALL_F32, every_row_differs
from tests.reference import FREESLIP, HOLD, NOSLIP, REPEAT, les_collide, moving, oracle_run, trt_collide
from tests.test_gpu_col_parked import PIN

Case = collections.namedtuple("Case", "k precision nx ny model param tau u geometry radius mask_seed profile schedule walls calls of "
                                      "trailing_pair plan strips strip_opts ckpt_plan")

MODELS = ("bgk", "les", "trt", "forced")
MODEL_BASE = {"bgk": 0, "les": 2, "trt": 4, "forced": 8}          # the kernels' strict Arith value (csrc/lbm_plan.hpp collision_models)
GEOMETRIES = ("disc", "random", "boundaries", "fluid")
MAGICS = (3.0 / 16.0, 1.0 / 4.0, 1.0 / 12.0)

# the pinned plans that are no key of helpers.PLANS: the fp64 64x40 regions (contracted, whole domains) and the fp32 64x48 regions (BGK)
PINNED = {
    "park10": dict(PIN, nt=0, ntl=1, alternate=1, deep=10),
    "park11": dict(PIN, nt=0, ntl=1, alternate=1, deep=11),
    "tall-f32": dict(TALL_F32, arith=0),
    "tall-f32-fast": dict(TALL_F32, arith=1),
}
PLAN_KEYS = [k for k in PLANS if k not in ("auto", "fast-auto")]      # (their measurement at initialise costs seconds and is covered elsewhere)
# what a checkpoint is handed to: one plan per kernel family and arithmetic mode
HANDOVER = {0: ["rowil-site-nt", "planar-pair8-nt", "planar-fuse3-8", "rowil-fuse4-nt-xcd", "rowil-deep6-nt", "rowil-col5-nt"],
            1: ["fast-site", "fast-planar-pair8", "fast-rowil-fuse3-12-xcd", "fast-rowil-fuse4-xcd", "fast-rowil-deep7", "fast-rowil-col6"]}


def plan_options(plan):
    return PINNED[plan] if plan in PINNED else PLANS[plan]


def contracted(plan):
    return int(plan_options(plan).get("arith", 0))


def family(plan):
    """The kernel family the plan pins: site / pair / fuse3 / fuse4 (LDS tiles), deep (LDS-filling tiles), col (64x24 / 64x32 regions in
    registers), park (64x40, fp64), tall (64x48, fp32)."""
    o = plan_options(plan)
    deep = o.get("deep", 0)
    if deep:
        return "park" if deep in (10, 11) else "tall" if deep == 8 else "col" if deep >= 6 else "deep"
    return "pair" if o.get("pair") else {1: "site", 2: "pair", 3: "fuse3", 4: "fuse4"}[o.get("fuse", 1)]


def options_of(case, plan=None):
    """The options of the case's context or group (plan: of the context a checkpoint is handed to)."""
    o = dict(plan_options(case.plan if plan is None else plan), trailing_pair=case.trailing_pair)
    if case.strips > 1:
        overlap, deep_halo, group_threads = case.strip_opts
        o.update(layout=1, alternate=0, overlap=overlap, deep_halo=deep_halo, group_threads=group_threads)
    return o


def mask_of(case):
    """The obstacle mask (ny, nx), or None for the analytic disc of the case's cylinder_radius."""
    nx, ny = case.nx, case.ny
    if case.geometry == "disc":
        return None
    m = np.zeros((ny, nx), np.uint8)
    if case.geometry == "random":
        m[np.random.default_rng(case.mask_seed).random((ny, nx)) < 0.03] = 1
    elif case.geometry == "boundaries":
        m[0:max(1, ny // 4), nx // 3:nx // 3 + max(1, nx // 8)] = 1          # a block standing on the south wall
        m[ny - 1, (2 * nx) // 3] = 1                                         # one cell in the top row,
        m[ny // 2, 0] = 1                                                    # one in column 0,
        m[(2 * ny) // 3, nx - 1] = 1                                         # one in the last column
    return m


def profile_of(case):
    return every_row_differs(case.ny, case.u) if case.profile else None


def schedule_of(case):
    """(table, HOLD or REPEAT) or None."""
    if case.schedule is None:
        return None
    n, mode, seed = case.schedule
    return np.random.default_rng(seed).uniform(0.2, 1.0, n), {"hold": HOLD, "repeat": REPEAT}[mode]


def physics_kw(case, **off):
    """oracle_run's keywords for the case; off: a keyword replaced (the feature-activity check switches one feature off)."""
    collide = {"bgk": None,
               "les": functools.partial(les_collide, cs=case.param),
               "trt": functools.partial(trt_collide, magic=case.param),
               "forced": functools.partial(guo_collide, force=case.param)}[case.model]
    kw = dict(mask=mask_of(case), u=profile_of(case), walls=case.walls, schedule=schedule_of(case), collide=collide,
              tau=case.tau, inlet_velocity=case.u, cylinder_radius=case.radius)
    kw.update(off)
    return kw


def context_kw(case):
    """Context's / Group's keywords for the case (without options=)."""
    kw = dict(tau=case.tau, inlet_velocity=case.u, cylinder_radius=case.radius, precision=case.precision, solid=mask_of(case),
              inlet_profile=profile_of(case), walls=case.walls)
    if case.schedule is not None:
        kw["inlet_schedule"] = (schedule_of(case)[0], case.schedule[1])
    if case.model != "bgk":
        kw[{"les": "smagorinsky", "trt": "trt_magic", "forced": "forcing"}[case.model]] = case.param
    return kw


def steps_of(case):
    return sum(case.calls)


def issued_calls(case):
    """The lengths of the step() calls as issued: with trailing_pair a call may end on a fused launch, which leaves no snapshot of the
    previous iteration, so the last call then ends with a single step."""
    calls = list(case.calls)
    if case.trailing_pair and calls[-1] > 1:
        calls[-1:] = [calls[-1] - 1, 1]
    return calls


def read_only(run):
    for a in (run.f_next, run.rho, run.ux, run.uy):
        a.flags.writeable = False
    return run


@functools.lru_cache(maxsize=None)
def reference_of(case):
    """The stepwise reference run of the case (tests/reference.py oracle_run with the model's operator); once, shared, read-only."""
    return read_only(oracle_run(case.nx, case.ny, steps_of(case), case.of, **physics_kw(case)))


@functools.lru_cache(maxsize=None)
def reference32_of(case):
    """reference_of in float32 (tests/numpy_oracle.py): what an fp32 context in strict arithmetic must equal bit for bit."""
    return read_only(oracle_run(case.nx, case.ny, steps_of(case), case.of, dtype=np.float32, **physics_kw(case)))


def _wall(rng):
    kind = int(rng.integers(0, 3))
    u_w = round(float(rng.uniform(-0.06, 0.06)), 4)
    return (NOSLIP, FREESLIP, moving(u_w))[kind]


def _cases(n, seed, precision):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        nx = int(rng.choice([rng.integers(2, 61), rng.integers(60, 201), rng.integers(200, 421), 54, 55, 56, 57, 64, 108, 112, 128, 130]))
        ny = int(rng.choice([rng.integers(2, 25), rng.integers(24, 81), rng.integers(80, 151), 22, 23, 24, 25, 44, 48, 50, 69, 70, 100]))
        model = MODELS[k % 4]
        tau = round(float(rng.uniform(0.56, 1.1)), 4)
        param = None
        if model == "les":
            param, tau = round(float(rng.uniform(0.1, 0.2)), 4), round(float(rng.uniform(0.52, 0.6)), 4)
        elif model == "trt":
            param = MAGICS[int(rng.integers(0, 3))]
        elif model == "forced":
            param = (round(float(rng.uniform(-5e-5, 5e-5)), 7), round(float(rng.uniform(-5e-5, 5e-5)), 7))
        u = round(float(rng.uniform(0.01, 0.08)), 4)
        geometry = GEOMETRIES[int(rng.integers(0, 4))]
        radius = (0.0, 0.1, 0.2)[int(rng.integers(0, 3))]
        mask_seed = int(rng.integers(0, 1 << 30))
        profile = int(rng.integers(0, 2))
        schedule = None
        if rng.integers(0, 2):
            schedule = (int(rng.integers(1, 41)), ("hold", "repeat")[int(rng.integers(0, 2))], int(rng.integers(0, 1 << 30)))
        walls = (_wall(rng), _wall(rng))
        steps, of = int(rng.integers(1, 151)), int(rng.integers(1, 46))
        cuts = sorted(set(int(c) for c in rng.integers(1, steps + 1, int(rng.integers(0, 3))) if c < steps))
        calls = tuple(b - a for a, b in zip([0] + cuts, cuts + [steps]))
        trailing_pair = int(rng.integers(0, 2))
        strips = 1
        if ny >= 40 and rng.random() < 0.6:
            strips = min(int(rng.integers(2, 5)), ny // 12)                 # (a strip with neighbours holds at least twelve rows)
        strip_opts = (int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 2))) if strips > 1 else None
        plan = PLAN_KEYS[int(rng.integers(0, len(PLAN_KEYS)))]
        # the tall shapes exist on whole domains only: fp64 64x40 (contracted; every model has them), fp32 64x48 (BGK alone has them,
        # and few fp32 cases are whole-domain BGK: most of those take one)
        tall = ("park10", "park11") if precision == "f64" else ("tall-f32", "tall-f32-fast") if model == "bgk" else None
        if strips == 1 and tall and rng.random() < (0.15 if precision == "f64" else 0.7):
            plan = tall[int(rng.integers(0, 2))]
        ckpt_plan = None
        if precision == "f64" and strips == 1 and len(calls) > 1 and rng.random() < 0.5:
            others = [p for p in HANDOVER[contracted(plan)] if family(p) != family(plan)]
            ckpt_plan = others[int(rng.integers(0, len(others)))]
        out.append(Case(k, precision, nx, ny, model, param, tau, u, geometry, radius, mask_seed, profile, schedule, walls, calls, of,
                        trailing_pair, plan, strips, strip_opts, ckpt_plan))
    return out


# ---- the deterministic lean-tile cases ---------------------------------------------------------------------------------------------
# 224x112 (fp32: 224x176) and 20 iterations with force samples every 16, the lattice and lengths of tests/test_gpu_geometry_edges.py:
# at least three tiles in each direction for every shape, so that interior tiles take the LEAN path (tests/test_feature_sweep_cpu.py
# counts them), two deep launches and a remainder; between a free-slip south and a moving north wall, so that the general tiles of the
# same launch carry features too
LEAN_NX, LEAN_NY, LEAN_NY_F32, LEAN_STEPS, LEAN_OF = 224, 112, 176, 20, 16
LEAN_WALLS = (FREESLIP, moving(0.05))
LEAN_MODELS = {"trt": dict(trt_magic=3.0 / 16.0), "forced": dict(forcing=(2e-5, -1e-5)), "les": dict(smagorinsky=0.17), "bgk": {}}
LEAN_PLANS = ["rowil-site-nt", "planar-fuse3-8", "rowil-deep6-nt", "rowil-col5-nt", "planar-col6-alt", "rowil-col7-alt", "fast-rowil-col6",
              "fast-planar-col5", "fast-rowil-deep7", "fast-rowil-col7", "park10", "park11"]          # helpers.ORACLE_PLANS and three more
LEAN_PLANS_F32 = [(m, p) for m in LEAN_MODELS for p in ("rowil-col5-nt", "fast-rowil-col6", "fast-rowil-col7")] + \
    [("bgk", "tall-f32"), ("bgk", "tall-f32-fast")]


def lean_kw(model):
    """Context's keywords of a lean-tile case (the default disc)."""
    return dict(LEAN_MODELS[model], tau=0.51 if model == "les" else 0.55, inlet_velocity=0.08, walls=LEAN_WALLS)


@functools.lru_cache(maxsize=None)
def lean_reference(model, walls=LEAN_WALLS):
    kw = lean_kw(model)
    collide = {"bgk": None, "les": functools.partial(les_collide, cs=kw.get("smagorinsky")),
               "trt": functools.partial(trt_collide, magic=kw.get("trt_magic")),
               "forced": functools.partial(guo_collide, force=kw.get("forcing"))}[model]
    return read_only(oracle_run(LEAN_NX, LEAN_NY, LEAN_STEPS, LEAN_OF, walls=walls, collide=collide, tau=kw["tau"],
                                inlet_velocity=kw["inlet_velocity"]))


def fp64_cases():
    return _cases(120, 20261020, "f64")


def fp32_cases():
    return _cases(40, 20261021, "f32")


def case_id(c):
    return "%d-%dx%d-%s-%s" % (c.k, c.nx, c.ny, c.model, c.plan) + ("-%dstrips" % c.strips if c.strips > 1 else "") + \
        ("-ckpt" if c.ckpt_plan else "")
