"""The stepwise reference of the inlet-schedule tests (test infrastructure): oracle_run of tests/reference.py with two changes.

The initial state is that of the profile u * s[0], and the numpy fix-up of the inlet column uses ur = u[rows] * s(t) at iteration t —
one IEEE multiplication in double, formed before 1 - ur and rho_bc * ur use it. The fix-up runs after o.boundaries() and keeps the
oracle's operation order, so strict fp64 plans must match it bit for bit. tests/test_inlet_schedule_cpu.py pins it to oracle_run."""
import numpy as np

from oracle.oracle import Oracle, make_params
from tests.reference import Run, feq_rows, link_forces

HOLD, REPEAT = 0, 1


def sched_index(t, n, mode):
    """Which entry iteration t takes: HOLD s[min(t, n - 1)], REPEAT s[t mod n] (the Python restatement of inlet_sched_index)."""
    return t % n if mode == REPEAT else min(t, n - 1)


def schedule_run(nx, ny, steps, of, *, s, mode=HOLD, mask=None, u=None, **params):
    """oracle_run with the inlet of row y at iteration t at u[y] * s(t) (u None: the uniform inlet_velocity of `params` on every
    row). Plain BGK; forces are [(t, fx, fy)] by link_forces."""
    o = Oracle(make_params(nx, ny, **params))
    if mask is not None:
        o.solid[:] = mask
    o.L.lbmo_initialise(o.h)
    solid = o.solid.astype(bool).copy()
    fluid = ~solid
    s = np.asarray(s, dtype=np.float64)
    u = np.full(ny, o.p.inlet_velocity, dtype=np.float64) if u is None else np.asarray(u, dtype=np.float64)
    u0 = u * s[0]                                 # interior fluid cells of row y start at f_eq(1, (u[y] * s[0], 0))
    fr = feq_rows(u0)
    for arr in (o.f_current, o.f_next):
        inner = arr[1:-1, 1:-1]
        inner[fluid] = np.broadcast_to(fr[:, None, :], (ny, nx, 9))[fluid]
    o.ux[fluid] = np.broadcast_to(u0[:, None], (ny, nx))[fluid]
    rows = np.nonzero(fluid[:, 0])[0]
    forces, bad = [], -1
    for t in range(steps):
        with np.errstate(all="ignore"):
            o.collide()
        if of and t % of == 0:
            forces.append((t,) + link_forces(o.f_next, solid))
        o.exchange_physical()
        o.stream()
        o.boundaries()
        ur = u[rows] * s[sched_index(t, len(s), mode)]
        f = o.f_current[rows + 1, 1, :]
        rho_bc = (f[:, 0] + f[:, 2] + f[:, 4] + 2.0 * (f[:, 3] + f[:, 6] + f[:, 7])) / (1.0 - ur)
        f[:, 1] = f[:, 3] + (2.0 / 3.0) * rho_bc * ur
        f[:, 5] = f[:, 7] - 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho_bc * ur
        f[:, 8] = f[:, 6] + 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho_bc * ur
        o.f_current[rows + 1, 1, :] = f
        o.rho[rows, 0] = rho_bc
        o.ux[rows, 0] = ur
        if not o.stable():
            bad = t
            break
    out = Run(o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy(), forces, bad, o.solid_count(), None)
    o.close()
    return out
