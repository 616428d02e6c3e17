"""The second generation of seeded cases of the feature sweep (test infrastructure; tests/test_gpu_feature_sweep2.py runs them on the
GPU, tests/test_feature_sweep2_cpu.py checks the generator and the references without one).

The first generation (tests/feature_cases.py: it never changes) predates periodic y, the two ports and the MRT collision. A Case2 is a
Case with three more fields: periodic (0 / 1), ports ((west, east) as the binding takes them) and bounds (None, or the explicit
(start, rows) strips of a group); the model set grows by "mrt" with param = (bulk_rate, magic). Half the cases are periodic, on the
strip plans of tests/test_gpu_periodic.py and on lattices down to the twelve rows a strip with neighbours needs, where the wrapped
tables wrap more than once; the other half are walled, on the first generation's plans, walls and heights. Both halves draw widths
from two columns up, port pairs at the magnitudes of tests/test_gpu_ports.py, groups of unequal strips with one of exactly twelve rows,
and (periodic) a body that the seam cuts. One reference loop runs them all: tests/periodic_reference.py periodic_run.

Besides the seeded cases: the smallest periodic lattices (SMALLEST), fixed, against every strip plan."""
import collections
import functools
import importlib

import numpy as np

from tests import feature_cases as fc
from tests.feature_cases import GEOMETRIES, HANDOVER, MAGICS, PLAN_KEYS, _wall, read_only
from tests.forcing_reference import guo_collide
from tests.helpers import PKG
from tests.mrt_reference import mrt_collide
from tests.periodic_reference import periodic_run, seam_profile
from tests.ports_reference import DEFAULT_PORTS, PRESSURE, VELOCITY
from tests.reference import NOSLIP, les_collide, trt_collide
from tests.test_gpu_periodic import PERIODIC_PLANS, TALL_F32

Case2 = collections.namedtuple("Case2", fc.Case._fields + ("periodic", "ports", "bounds"))

MODELS = fc.MODELS + ("mrt",)
MODEL_BASE = dict(fc.MODEL_BASE, mrt=16)                             # (csrc/lbm_plan.hpp collision_models)
ROTATION = ("bgk", "les", "mrt", "trt", "forced", "mrt")             # the models in rotation, MRT in one third of the cases
GEOMETRIES2 = GEOMETRIES + ("seam",)                                 # (seam: periodic cases only)
NX_FIXED = [2, 3, 54, 55, 56, 57, 63, 64, 65, 108, 112, 128, 130]
NY_PERIODIC = [12, 13, 15, 16, 17, 23, 24, 25, 31, 32, 33, 44, 48, 50, 69, 70]
# the tall fp32 regions on a periodic context (tests/test_gpu_periodic.py TALL_F32, by arithmetic mode)
PERIODIC_TALL = {"tall-f32": TALL_F32[0], "tall-f32-fast": TALL_F32[1]}
PERIODIC_KEYS = list(PERIODIC_PLANS)
PERIODIC_FAMILIES = ("site", "pair", "fuse3", "deep", "col")         # every family a strip may run (fp32: and "tall")


def plan_options(plan, periodic):
    """The options a plan's name pins: a periodic case names a strip plan of tests/test_gpu_periodic.py, a walled one a plan of the
    first generation (some names are keys of both tables)."""
    if periodic:
        return PERIODIC_TALL[plan] if plan in PERIODIC_TALL else PERIODIC_PLANS[plan]
    return fc.plan_options(plan)


def contracted(plan, periodic):
    return int(plan_options(plan, periodic).get("arith", 0))


def family(plan, periodic):
    """feature_cases.family of the plan's options (a strip plan with pair=1 is "pair")."""
    o = plan_options(plan, periodic)
    deep = o.get("deep", 0)
    if deep:
        return "park" if deep in (10, 11) else "tall" if deep == 8 else "col" if deep >= 6 else "deep"
    return "pair" if o.get("pair") else {1: "site", 2: "pair", 3: "fuse3", 4: "fuse4"}[o.get("fuse", 1)]


def grouped(case):
    """A Group runs the case (a linked ring of one strip included), not a Context."""
    return case.strips > 1 or case.bounds is not None


def bounds_of(case):
    """The (start, rows) strips of a grouped case: the explicit ones, or the even split of the binding."""
    if case.bounds is not None:
        return [tuple(b) for b in case.bounds]
    return importlib.import_module(PKG + ".strips").partition_rows(case.ny, case.strips)


def options_of(case, plan=None):
    """The options of the case's context or group (plan: of the context a checkpoint is handed to)."""
    o = dict(plan_options(case.plan if plan is None else plan, case.periodic), trailing_pair=case.trailing_pair)
    if grouped(case):
        overlap, deep_halo, group_threads = case.strip_opts
        o.update(layout=1, alternate=0, overlap=overlap, deep_halo=deep_halo, group_threads=group_threads)
    return o


def seam_block(nx, ny):
    """The seam geometry: a block over rows ny-k .. ny-1 and 0 .. k-1, k = min(3, ny // 4), which the seam cuts; one solid cell in
    column 0 and one in column nx - 1."""
    m = np.zeros((ny, nx), np.uint8)
    k = min(3, ny // 4)
    x0 = nx // 3
    m[ny - k:, x0:x0 + max(1, nx // 8)] = 1
    m[:k, x0:x0 + max(1, nx // 8)] = 1
    m[ny // 2, 0] = 1
    m[(2 * ny) // 3, nx - 1] = 1
    return m


def mask_of(case):
    return seam_block(case.nx, case.ny) if case.geometry == "seam" else fc.mask_of(case)


profile_of, schedule_of, steps_of, issued_calls = fc.profile_of, fc.schedule_of, fc.steps_of, fc.issued_calls


def collide_of(case):
    return {"bgk": lambda: None,
            "les": lambda: functools.partial(les_collide, cs=case.param),
            "trt": lambda: functools.partial(trt_collide, magic=case.param),
            "forced": lambda: functools.partial(guo_collide, force=case.param),
            "mrt": lambda: functools.partial(mrt_collide, bulk_rate=case.param[0], magic=case.param[1])}[case.model]()


def physics_kw(case, **off):
    """periodic_run's keywords for the case; off: a keyword replaced (the feature-activity check switches one feature off)."""
    kw = dict(periodic=bool(case.periodic), ports=case.ports, mask=mask_of(case), u=profile_of(case), walls=case.walls,
              schedule=schedule_of(case), collide=collide_of(case), tau=case.tau, inlet_velocity=case.u, cylinder_radius=case.radius)
    kw.update(off)
    return kw


def context_kw(case):
    """Context's / Group's keywords for the case (without options=)."""
    kw = dict(tau=case.tau, inlet_velocity=case.u, cylinder_radius=case.radius, precision=case.precision, solid=mask_of(case),
              inlet_profile=profile_of(case), ports=case.ports)
    if case.periodic:
        kw["periodic_y"] = True
    else:
        kw["walls"] = case.walls
    if case.schedule is not None:
        kw["inlet_schedule"] = (schedule_of(case)[0], case.schedule[1])
    if case.model != "bgk":
        kw[{"les": "smagorinsky", "trt": "trt_magic", "forced": "forcing", "mrt": "mrt"}[case.model]] = case.param
    return kw


@functools.lru_cache(maxsize=None)
def reference_of(case):
    """The stepwise reference run of the case (periodic_run with the model's operator); once, shared, read-only."""
    return read_only(periodic_run(case.nx, case.ny, steps_of(case), case.of, **physics_kw(case)))


@functools.lru_cache(maxsize=None)
def reference32_of(case):
    """reference_of in float32: what an fp32 context in strict arithmetic must equal bit for bit."""
    return read_only(periodic_run(case.nx, case.ny, steps_of(case), case.of, dtype=np.float32, **physics_kw(case)))


def _bounds(rng, ny, n):
    """n unequal strips of at least twelve rows each, one of them of exactly twelve."""
    rows = [12] * n
    twelve = int(rng.integers(0, n))
    free = [j for j in range(n) if j != twelve]
    extra = ny - 12 * n
    cuts = sorted(int(c) for c in rng.integers(0, extra + 1, len(free) - 1))
    for j, (a, b) in zip(free, zip([0] + cuts, cuts + [extra])):
        rows[j] += b - a
    starts = [sum(rows[:j]) for j in range(n)]
    return tuple(zip(starts, rows))


def _cases2(n, seed, precision):
    rng = np.random.default_rng(seed)
    out = []
    heights = [int(v) for v in rng.permutation(len(NY_PERIODIC) + 1)]     # the periodic heights in turn, in a drawn order
    for k in range(n):
        model = ROTATION[k % 6]
        periodic = (k // 6 + k) % 2                                  # half the cases, and half of every model's
        nx = int(rng.choice(NX_FIXED + [int(rng.integers(2, 61)), int(rng.integers(60, 261))]))
        if periodic:
            ny = (NY_PERIODIC + [int(rng.integers(12, 151))])[heights[(k // 2) % len(heights)]]
            walls = (NOSLIP, NOSLIP)
        else:
            ny = int(rng.choice([rng.integers(2, 25), rng.integers(24, 81), rng.integers(80, 151), 22, 23, 24, 25, 44, 48, 50, 69, 70, 100]))
            walls = (_wall(rng), _wall(rng))
        tau = round(float(rng.uniform(0.56, 1.1)), 4)
        param = None
        if model == "les":
            param, tau = round(float(rng.uniform(0.1, 0.2)), 4), round(float(rng.uniform(0.52, 0.6)), 4)
        elif model == "trt":
            param = MAGICS[int(rng.integers(0, 3))]
        elif model == "forced":
            param = (round(float(rng.uniform(-5e-5, 5e-5)), 7), round(float(rng.uniform(-5e-5, 5e-5)), 7))
        elif model == "mrt":
            param = (round(float(rng.uniform(0.6, 1.9)), 4), MAGICS[int(rng.integers(0, 3))])
        u = round(float(rng.uniform(0.01, 0.08)), 4)
        # the ports: a quarter of the cases keep the default pair; else either kind at either end
        ports = DEFAULT_PORTS
        if rng.random() >= 0.25:
            west = VELOCITY if rng.integers(0, 2) else (PRESSURE, round(float(rng.uniform(1.0, 1.015)), 4))
            east = (PRESSURE, round(float(rng.uniform(0.985, 1.0)), 4)) if rng.integers(0, 2) else (VELOCITY, round(float(rng.uniform(0.0, 0.03)), 4))
            ports = (west, east)
        geometry = GEOMETRIES2[int(rng.integers(0, 5 if periodic else 4))]
        radius = (0.0, 0.1, 0.2)[int(rng.integers(0, 3))]
        mask_seed = int(rng.integers(0, 1 << 30))
        profile = int(rng.integers(0, 2))
        schedule = None
        if rng.integers(0, 2):
            schedule = (int(rng.integers(1, 41)), ("hold", "repeat")[int(rng.integers(0, 2))], int(rng.integers(0, 1 << 30)))
        if ports[0] != VELOCITY:                                     # (lbm_initialise refuses both beside a west pressure port)
            profile, schedule = 0, None
        steps, of = int(rng.integers(1, 101)), int(rng.integers(1, 46))
        cuts = sorted(set(int(c) for c in rng.integers(1, steps + 1, int(rng.integers(0, 3))) if c < steps))
        calls = tuple(b - a for a, b in zip([0] + cuts, cuts + [steps]))
        trailing_pair = int(rng.integers(0, 2))
        strips, bounds = 1, None
        if ny >= (24 if periodic else 40) and rng.random() < 0.6:
            strips = min(int(rng.integers(2, 5)), ny // 12)          # (a strip with neighbours, or on a ring, holds at least twelve rows)
            if periodic and rng.random() < 0.15:
                strips, bounds = 1, ((0, ny),)                       # a linked ring of one strip
            elif rng.integers(0, 2):
                bounds = _bounds(rng, ny, strips)
        group = strips > 1 or bounds is not None
        strip_opts = (int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 2))) if group else None
        if periodic:
            among = [p for p in PERIODIC_KEYS if family(p, 1) == PERIODIC_FAMILIES[(k // 2) % 5]]          # the families in turn
            plan = among[int(rng.integers(0, len(among)))]
            tall = ("tall-f32", "tall-f32-fast") if precision == "f32" and model == "bgk" else None
            chance = 0.5
        else:
            plan = PLAN_KEYS[int(rng.integers(0, len(PLAN_KEYS)))]
            # the tall shapes exist on whole domains only: fp64 64x40 (contracted; every model but MRT has them), fp32 64x48 (BGK alone)
            tall = (("park10", "park11") if model != "mrt" else None) if precision == "f64" else ("tall-f32", "tall-f32-fast") if model == "bgk" else None
            chance = 0.15 if precision == "f64" else 0.7
        if not group and tall and rng.random() < chance:
            plan = tall[int(rng.integers(0, 2))]
        ckpt_plan = None
        if precision == "f64" and not group and len(calls) > 1 and rng.random() < 0.5:
            table = [p for p in PERIODIC_KEYS if contracted(p, 1) == contracted(plan, 1)] if periodic else HANDOVER[contracted(plan, 0)]
            others = [p for p in table if family(p, periodic) != family(plan, periodic)]
            ckpt_plan = others[int(rng.integers(0, len(others)))]
        out.append(Case2(k, precision, nx, ny, model, param, tau, u, geometry, radius, mask_seed, profile, schedule, walls, calls, of,
                         trailing_pair, plan, strips, strip_opts, ckpt_plan, periodic, ports, bounds))
    return out


def fp64_cases():
    return _cases2(96, 20261105, "f64")


def fp32_cases():
    return _cases2(32, 20261282, "f32")


def case_id(c):
    return "%d-%dx%d-%s-%s%s" % (c.k, c.nx, c.ny, c.model, "periodic-" if c.periodic else "", c.plan) + \
        ("-%dstrips" % len(bounds_of(c)) if grouped(c) else "") + ("-ckpt" if c.ckpt_plan else "")


# ---- the smallest periodic lattices, fixed ---------------------------------------------------------------------------------------------
# ny below the pad of sixteen rows (the wrapped tables wrap more than once, a face's twelve ghost rows are the whole lattice), nx
# narrower than a tile and with a partial last column of regions; the seam geometry, an inlet profile that differs on every row
SMALLEST = [(2, 12), (3, 13), (64, 12), (65, 15), (57, 16), (130, 17)]
SMALLEST_TAU, SMALLEST_U0 = 0.6, 0.05
SMALLEST_CALLS = [(5, 3), (1, 3), (8, 3)]                            # 14 iterations, forces every third
SMALLEST_STEPS, SMALLEST_OF = 14, 3
SMALLEST_F32_PLANS = ["site", "fuse3", "deep1", "deep7", "tall-f32"]
# 65x15 and 130x17 a second time, with MRT and a pressure / pressure port pair
SMALLEST_VARIANTS = {
    "plain": (dict(), dict()),
    "mrt-pressure-pair": (dict(mrt=(1.4, 3.0 / 16.0), ports=((PRESSURE, 1.004), (PRESSURE, 0.996))),
                          dict(collide=functools.partial(mrt_collide, bulk_rate=1.4, magic=3.0 / 16.0), ports=((PRESSURE, 1.004), (PRESSURE, 0.996)))),
}
SMALLEST_CASES = [(nx, ny, "plain") for nx, ny in SMALLEST] + [(65, 15, "mrt-pressure-pair"), (130, 17, "mrt-pressure-pair")]
# (lattice, plan) pairs that the library refuses with LBM_ERR_ARG under a rule DESIGN.md states, with the refusal's text: none
SMALLEST_REFUSED = {}


def smallest_inputs(nx, ny, variant, roll=0):
    """(Context's keywords, periodic_run's keywords) of a smallest-lattice case, mask and profile rolled by `roll` rows."""
    ctx_kw, ref_kw = SMALLEST_VARIANTS[variant]
    mask = np.roll(seam_block(nx, ny), roll, axis=0)
    u = None if "ports" in ctx_kw else np.roll(seam_profile(ny, SMALLEST_U0), roll)          # (a west pressure port takes no profile)
    return (dict(ctx_kw, tau=SMALLEST_TAU, inlet_velocity=SMALLEST_U0, solid=mask, inlet_profile=u, periodic_y=True),
            dict(ref_kw, tau=SMALLEST_TAU, inlet_velocity=SMALLEST_U0, mask=mask, u=u))


@functools.lru_cache(maxsize=None)
def smallest_reference(nx, ny, variant, precision="f64", roll=0):
    dtype = {"f32": np.float32, "f64": np.float64}[precision]
    return read_only(periodic_run(nx, ny, SMALLEST_STEPS, SMALLEST_OF, dtype=dtype, **smallest_inputs(nx, ny, variant, roll)[1]))
