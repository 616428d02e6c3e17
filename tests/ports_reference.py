"""The reference of the two ports (lbm_set_port) for the GPU and CPU port tests (test infrastructure): `boundaries` of tests/reference.py
restated with the table of include/lbm_hip.h in place of the velocity inlet and the rho = 1 outlet, and the loop of oracle_run restated
around it. numpy, fp64, IEEE, one operation per operation of the table in the order written: strict plans must match it bit for bit.
With the default ports it is oracle_run to the bit (tests/test_ports_cpu.py)."""
import numpy as np

from tests.reference import NOSLIP, OPP, close_run, link_forces, open_run, wall_kind_k, wall_rule

VELOCITY, PRESSURE = "velocity", "pressure"
DEFAULT_PORTS = (VELOCITY, (PRESSURE, 1.0))


def port_of(p, default):
    """(kind name, value) of a port as the binding takes it: None = the default, "velocity" = the west velocity port."""
    if p is None:
        p = default
    if isinstance(p, str):
        assert p == VELOCITY
        return VELOCITY, 0.0
    kind, v = p
    assert kind in (VELOCITY, PRESSURE)
    return kind, float(v)


def port_rule(f, side, kind, given):
    """The table of include/lbm_hip.h (lbm_set_port) on cells f[n, 9], in place; side 0: west, 1: east; `given`: the density of a
    pressure port, the velocity of a velocity port (a scalar, or one value per cell). Returns (rho, u) of the rule."""
    if side == 0:
        S = f[:, 0] + f[:, 2] + f[:, 4] + 2.0 * (f[:, 3] + f[:, 6] + f[:, 7])
        if kind == PRESSURE:
            rho = np.full_like(S, given); u = 1.0 - S / rho
        else:
            u = np.broadcast_to(np.asarray(given, dtype=f.dtype), S.shape).copy(); rho = S / (1.0 - u)
        f[:, 1] = f[:, 3] + (2.0 / 3.0) * rho * u
        f[:, 5] = f[:, 7] - 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho * u
        f[:, 8] = f[:, 6] + 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho * u
    else:
        S = f[:, 0] + f[:, 2] + f[:, 4] + 2.0 * (f[:, 1] + f[:, 5] + f[:, 8])
        if kind == PRESSURE:
            rho = np.full_like(S, given); u = -1.0 + S / rho
        else:
            u = np.full_like(S, given); rho = S / (1.0 + u)
        f[:, 3] = f[:, 1] - (2.0 / 3.0) * rho * u
        f[:, 6] = f[:, 8] - 0.5 * (f[:, 2] - f[:, 4]) - (1.0 / 6.0) * rho * u
        f[:, 7] = f[:, 5] + 0.5 * (f[:, 2] - f[:, 4]) - (1.0 / 6.0) * rho * u
    assert rho.dtype == u.dtype == f.dtype, "the port rule left " + str(f.dtype)      # (the caller's assignments would cast silently)
    return rho, u


def boundaries(o, solid, walls, u, ports):
    """tests/reference.py `boundaries` with the two ports: bottom, top, west, east, solid cells, in that order; rho / ux / uy of the
    port columns are (rho, u, 0) of the rule. u: the west velocity of every row at this iteration (read by a west velocity port)."""
    fc = o.f_current
    ny, nx = solid.shape
    fluid = ~solid
    for side, gy, y in ((0, 1, 0), (1, ny, ny - 1)):
        kind, k = wall_kind_k(walls[side])
        cols = np.nonzero(fluid[y])[0] + 1
        fc[gy, cols, :] = wall_rule(fc[gy, cols, :], side, kind, k)
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


def ports_run(nx, ny, steps, of, *, ports=DEFAULT_PORTS, mask=None, u=None, walls=(NOSLIP, NOSLIP), schedule=None, collide=None,
              keep_f_current=False, dtype=np.float64, backend=None, **params):
    """tests/reference.py oracle_run with ports = (west, east): west "velocity" or ("pressure", rho), east ("pressure", rho) or
    ("velocity", u), None in either place the default. The initial state stays oracle_run's. Returns a Run."""
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
                forces.append((t,) + link_forces(o.f_next, solid))
            o.exchange_physical()
            o.stream()
            boundaries(o, solid, walls, u_at(t), ports)
        if not o.stable():
            bad = t
            break
    return close_run(o, solid, forces, bad, tmax, collide, keep_f_current)


# ---- the pressure-driven channel of the physics checks (tests/test_ports_cpu.py, tests/test_gpu_ports.py) -----------------------------
CHANNEL = dict(nx=48, ny=17, tau=1.0, ports=((PRESSURE, 1.005), (PRESSURE, 0.995)))
_channel_runs = {}


def channel_run(steps):
    """The all-fluid 48x17 channel from rest between no-slip walls under the density difference 1.005 - 0.995, after `steps`
    iterations; once per length, shared, read-only."""
    if steps not in _channel_runs:
        nx, ny = CHANNEL["nx"], CHANNEL["ny"]
        run = ports_run(nx, ny, steps, 0, ports=CHANNEL["ports"], mask=np.zeros((ny, nx), np.uint8), tau=CHANNEL["tau"], inlet_velocity=0.0)
        for a in (run.f_next, run.rho, run.ux, run.uy):
            a.flags.writeable = False
        _channel_runs[steps] = run
    return _channel_runs[steps]
