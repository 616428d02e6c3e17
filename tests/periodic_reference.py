"""The reference of periodic top and bottom boundaries (lbm_set_periodic_y) for the GPU and CPU periodic tests (test infrastructure):
oracle_run's loop (tests/reference.py; with the two ports of tests/ports_reference.py) with three changes: after
o.exchange_physical() the edge rows become the opposite ghost rows (the oracle's own strip exchange, with itself as both neighbours);
`boundaries` without the wall loop; `link_forces` with the y-neighbour taken by np.roll. numpy, fp64, IEEE: strict plans must match it
bit for bit. With periodic=False it is oracle_run to the bit (tests/test_periodic_cpu.py)."""
import functools

import numpy as np

from tests.ports_reference import DEFAULT_PORTS, VELOCITY, port_of, port_rule
from tests.ports_reference import boundaries as walled_boundaries
from tests.reference import CX, CY, NOSLIP, OPP, close_run, link_forces, open_run


def periodic_boundaries(o, solid, u, ports):
    """tests/ports_reference.py `boundaries` without the wall loop: west, east, solid cells."""
    fc = o.f_current
    ny, nx = solid.shape
    fluid = ~solid
    for side, x in ((0, 0), (1, nx - 1)):
        kind, value = ports[side]
        rows = np.nonzero(fluid[:, x])[0]
        f = fc[rows + 1, x + 1, :]
        rho, ux = port_rule(f, side, kind, u[rows] if (side == 0 and kind == VELOCITY) else value)
        fc[rows + 1, x + 1, :] = f
        o.rho[rows, x] = rho; o.ux[rows, x] = ux; o.uy[rows, x] = 0.0
    inner = fc[1:-1, 1:-1]
    inner[solid] = inner[solid][:, OPP]
    o.ux[solid] = 0.0; o.uy[solid] = 0.0


def periodic_link_forces(f_next, solid):
    """link_forces with the lattice repeated in y: a fluid cell (x, y) whose neighbour (x + cx, (y + cy) mod ny) is solid contributes
    2 c_i f_i; the x-neighbour must lie in the domain, as ever."""
    ny, nx = solid.shape
    fx = fy = 0.0
    f = f_next[1:-1, 1:-1]
    for i in range(1, 9):
        rolled = np.roll(solid, -CY[i], axis=0)               # rolled[y] = solid[(y + cy) mod ny]
        nb = np.zeros_like(solid)
        xs, xd = (slice(CX[i], None), slice(0, nx - CX[i])) if CX[i] >= 0 else (slice(0, nx + CX[i]), slice(-CX[i], None))
        nb[:, xd] = rolled[:, xs]
        sel = nb & ~solid
        s = float(np.sum(f[..., i][sel].astype(np.float64)))      # (k_forces widens each population and sums in double)
        fx += 2.0 * CX[i] * s
        fy += 2.0 * CY[i] * s
    return fx, fy


def periodic_run(nx, ny, steps, of, *, periodic=True, ports=DEFAULT_PORTS, mask=None, u=None, walls=(NOSLIP, NOSLIP), schedule=None,
                 collide=None, keep_f_current=False, dtype=np.float64, backend=None, **params):
    """oracle_run (ports_run) on a lattice that is periodic in y; the keywords are theirs. `walls` counts with periodic=False only."""
    if isinstance(walls, str):
        walls = (walls, walls)
    ports = (port_of(ports[0], DEFAULT_PORTS[0]), port_of(ports[1], DEFAULT_PORTS[1]))
    o, solid, u_at = open_run(nx, ny, dtype, backend, mask, u, schedule, **params)
    tau = o.p.tau
    forces, bad, tmax = [], -1, None
    for t in range(steps):
        with np.errstate(all="ignore"):
            got = o.collide() if collide is None else collide(o, tau)
            if got is not None:
                tmax = max(tau if tmax is None else tmax, got)
            if of and t % of == 0:
                forces.append((t,) + (periodic_link_forces if periodic else link_forces)(o.f_next, solid))
            o.exchange_physical()
            if periodic:
                o.set_ghost_row(0, o.edge_row(1))
                o.set_ghost_row(1, o.edge_row(0))
            o.stream()
            u_t = u_at(t)
            if periodic:
                periodic_boundaries(o, solid, u_t, ports)
            else:
                walled_boundaries(o, solid, walls, u_t, ports)
        if not o.stable():
            bad = t
            break
    return close_run(o, solid, forces, bad, tmax, collide, keep_f_current)


# ---- the inputs of the periodic tests: 200x72, tau 0.6, 60 iterations ----------------------------------------------------------------
NX, NY, TAU, STEPS, OF, U0 = 200, 72, 0.6, 60, 5, 0.05


def seam_mask(nx=NX, ny=NY):
    """A 6x6 body across the seam (rows ny-3 .. ny-1 and 0 .. 2), a 4x6 block mid-channel and one-cell obstacles on row 0 and row ny-1."""
    m = np.zeros((ny, nx), np.uint8)
    m[ny - 3:, 40:46] = 1
    m[:3, 40:46] = 1
    m[ny // 2 - 2:ny // 2 + 2, 90:96] = 1
    m[0, 130] = 1
    m[ny - 1, 150] = 1
    return m


def seam_profile(ny=NY, u0=U0):
    """An inlet velocity that differs on every row (and between row 0 and row ny - 1)."""
    y = np.arange(ny, dtype=np.float64)
    return u0 * (0.6 + 0.4 * np.sin(2.0 * np.pi * (y + 0.25) / ny) + 0.003 * y)


def read_only(run):
    for a in (run.f_next, run.rho, run.ux, run.uy):
        a.flags.writeable = False
    return run


@functools.lru_cache(maxsize=None)
def seam_reference(roll=0, fluid=False, periodic=True):
    """The reference run on the inputs above, rolled by `roll` rows (fluid: no obstacle and the uniform inlet, a uniform stream); once
    per parameter set, shared, read-only."""
    mask = np.zeros((NY, NX), np.uint8) if fluid else np.roll(seam_mask(), roll, axis=0)
    u = None if fluid else np.roll(seam_profile(), roll)
    return read_only(periodic_run(NX, NY, STEPS, OF, periodic=periodic, mask=mask, u=u, tau=TAU, inlet_velocity=U0))
