"""The cases of the fp32-against-reference tests (test infrastructure): tests/test_gpu_f32_oracle.py runs them on the GPU,
tests/test_f32_reference_cpu.py computes their float32 floors and checks them without one.

A case is a lattice, a length, the keywords of its reference loop and the keywords of the Context (or Group) that must reproduce it.
reference(name, "f32") is the float32 run of tests/reference.py (on tests/numpy_oracle.py), which the strict fp32 plans must equal bit
for bit; reference(name, "f64") the fp64 run of the same physics on the C oracle. floors(name) is the one against the other: what
float32 rounding alone does to the case, and the unit of the bar of the contracted fp32 plans (4 floors: test_gpu_f32_oracle.py)."""
import collections
import functools

import numpy as np

from tests import feature_cases as fc
from tests.forcing_reference import guo_collide
from tests.helpers import every_row_differs, linf_rel
from tests.mrt_reference import mrt_collide
from tests.periodic_reference import NX as P_NX, NY as P_NY, OF as P_OF, STEPS as P_STEPS, TAU as P_TAU, U0 as P_U0
from tests.periodic_reference import periodic_run, seam_mask, seam_profile
from tests.ports_reference import ports_run
from tests.reference import FREESLIP, REPEAT, les_collide, moving, oracle_run, trt_collide
from tests.test_gpu_ports import EDGE_PAIRS, PAIRS, edge_mask

Case = collections.namedtuple("Case", "name nx ny calls model loop ref_kw ctx_kw")

# ---- the collision models: Context's keywords, the reference's operator, the strict Arith value of the kernels --------------------------
MODELS = {
    "bgk": ({}, None),
    "les": (dict(smagorinsky=0.17), functools.partial(les_collide, cs=0.17)),
    "trt": (dict(trt_magic=3.0 / 16.0), functools.partial(trt_collide, magic=3.0 / 16.0)),
    "forced": (dict(forcing=(2e-5, -1e-5)), functools.partial(guo_collide, force=(2e-5, -1e-5))),
    "mrt": (dict(mrt=(1.0, 3.0 / 16.0)), functools.partial(mrt_collide, bulk_rate=1.0, magic=3.0 / 16.0)),
}
MODEL_BASE = dict(fc.MODEL_BASE, mrt=16)

# 130x100, 23 iterations: three deep launches and a remainder at every depth, the last 64-wide region holds two columns, the 48-row
# tall regions get a partial band
NX, NY, STEPS, OF = 130, 100, 23, 8
WALLS = (FREESLIP, moving(0.05))
U = 0.05
LOOPS = {"oracle": oracle_run, "ports": ports_run, "periodic": periodic_run}
CASES = {}


def add(name, nx, ny, calls, model="bgk", loop="oracle", mask=None, u=None, schedule=None, walls=WALLS, ports=None, tau=0.6, u_in=U):
    """One case: `calls` = [(iterations, force output frequency)] as issued to step(); the reference runs their sum at the first
    call's frequency (the calls of a case share it)."""
    ckw, collide = MODELS[model]
    ref_kw = dict(mask=mask, u=u, schedule=schedule, collide=collide, tau=tau, inlet_velocity=u_in)
    ctx_kw = dict(ckw, tau=tau, inlet_velocity=u_in, solid=mask, inlet_profile=u)
    if schedule is not None:
        ctx_kw["inlet_schedule"] = (schedule[0], "repeat" if schedule[1] == REPEAT else "hold")
    if loop == "periodic":
        ctx_kw["periodic_y"] = True
    else:
        ref_kw["walls"] = walls
        ctx_kw["walls"] = walls
    if ports is not None:
        ref_kw["ports"] = ports
        ctx_kw["ports"] = ports
    assert len(set(of for _, of in calls)) == 1 and name not in CASES
    CASES[name] = Case(name, nx, ny, tuple(calls), model, loop, ref_kw, ctx_kw)
    return name


def sweep_mask(geometry, nx, ny, seed=20261021):
    """A mask of tests/feature_cases.py mask_of on another lattice."""
    blank = fc.Case(*[None] * len(fc.Case._fields))
    return fc.mask_of(blank._replace(nx=nx, ny=ny, geometry=geometry, mask_seed=seed))


FAMILIES = {m: add("families-" + m, NX, NY, [(STEPS, OF)], m, tau=0.52 if m == "les" else 0.6) for m in MODELS}
# the register kernel's LEAN path (interior tiles): the lattice, length and physics of the sweep's lean-tile cases
LEAN = {m: add("lean-" + m, fc.LEAN_NX, fc.LEAN_NY_F32, [(fc.LEAN_STEPS, fc.LEAN_OF)], m, walls=fc.LEAN_WALLS,
               tau=0.51 if m == "les" else 0.55, u_in=0.08) for m in MODELS}
FEATURES = [add("ports-" + k, NX, 70, [(STEPS, OF)], loop="ports", ports=v) for k, v in PAIRS.items()]
FEATURES += [add("edges-%dx%d-%d" % (nx, ny, k), nx, ny, [(STEPS, OF)], loop="ports", mask=edge_mask(nx, ny), ports=EDGE_PAIRS[k])
             for nx, ny in ((65, 25), (129, 49)) for k in (0, 1)]
FEATURES += [add("smallest-%dx%d-%d" % (nx, ny, k), nx, ny, [(7, OF)], loop="ports", mask=np.zeros((ny, nx), np.uint8), ports=EDGE_PAIRS[k])
             for nx, ny in ((2, 2), (3, 2)) for k in (0, 1)]
# a velocity per row times a factor per iteration: the product is formed in the element type on the device, not cast from a double product
FEATURES.append(add("rows-schedule", NX, NY, [(STEPS, OF)], u=every_row_differs(NY, U),
                    schedule=(np.random.default_rng(7).uniform(0.2, 1.0, 7), REPEAT)))
FEATURES += [add("mask-" + g, NX, NY, [(STEPS, OF)], mask=sweep_mask(g, NX, NY)) for g in ("random", "boundaries")]
# periodic y: the body across the seam and the profile of tests/periodic_reference.py, in the calls of tests/test_gpu_periodic.py
PERIODIC = add("periodic-seam", P_NX, P_NY, [(13, P_OF), (1, P_OF), (20, P_OF), (26, P_OF)], loop="periodic", mask=seam_mask(),
               u=seam_profile(), tau=P_TAU, u_in=P_U0)
assert sum(n for n, _ in CASES[PERIODIC].calls) == P_STEPS


def steps_of(case):
    return sum(n for n, _ in case.calls)


def read_only(run):
    for a in (run.f_next, run.rho, run.ux, run.uy, run.solid):
        a.flags.writeable = False
    return run


@functools.lru_cache(maxsize=None)
def reference(name, precision, steps=None):
    """The reference run of a case in "f32" or "f64" (steps: of another length than the case's); once, shared, read-only."""
    c = CASES[name]
    dtype = {"f32": np.float32, "f64": np.float64}[precision]
    return read_only(LOOPS[c.loop](c.nx, c.ny, steps_of(c) if steps is None else steps, c.calls[0][1], dtype=dtype, **c.ref_kw))


def errors(f_next, macros, ref):
    """(err_f, err_rho, err_u) of a result against a reference run: f_next relative to max |f_ref|, rho absolute, both velocity components
    relative to the reference's largest speed."""
    rho, ux, uy = macros
    uscale = float(np.max(np.sqrt(ref.ux.astype(np.float64) ** 2 + ref.uy.astype(np.float64) ** 2)))
    return (linf_rel(f_next, ref.f_next), float(np.max(np.abs(np.asarray(rho, np.float64) - ref.rho))),
            max(linf_rel(ux, ref.ux, uscale), linf_rel(uy, ref.uy, uscale)))


@functools.lru_cache(maxsize=None)
def floors(name):
    """(floor_f, floor_rho, floor_u): the float32 reference of the case against its float64 reference."""
    r32, r64 = reference(name, "f32"), reference(name, "f64")
    return errors(r32.f_next, (r32.rho, r32.ux, r32.uy), r64)


def floors_of_runs(r32, r64):
    return errors(r32.f_next, (r32.rho, r32.ux, r32.uy), r64)


# A contracted fp32 run (one reciprocal of rho with a Newton step, FMAs) is another float32 rounding history of the same formulas. On the
# CPU a deliberately different float32 history (one reciprocal of rho, another bracket order, f + w (feq - f)) lands between 0.4 and
# 2.3 times the strict floor against the float64 reference; 4 leaves room over that and is 2.5 to 6 times tighter than 2e-5 / 2e-4.
FACTOR = 4.0


def contracted_problems(err, floor):
    """What of (err_f, err_rho, err_u) of a contracted fp32 run against the float64 reference exceeds FACTOR float32 floors of the
    case. (Written so that a NaN fails.)"""
    return ["%s off by %.3g, %.2f floors of %.3g (bar %g floors)" % (k, e, e / f if f > 0 else float("inf"), f, FACTOR)
            for k, e, f in zip(("f_next", "rho", "u"), err, floor) if not e <= FACTOR * f]
