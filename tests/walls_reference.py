"""The stepwise reference run of the wall tests (lbm_set_wall; test infrastructure, like tests/reference.py).

The loop is oracle_run's of tests/reference.py — o.collide() or a numpy collision operator, link_forces, o.exchange_physical(),
o.stream(), o.stable() — with a numpy restatement of ALL of lbmo_boundaries (oracle/lbm_oracle.c) in place of o.boundaries(): the two
walls with their kind and k, the inlet with u[y], the outlet, the solid reversal, and rho / ux / uy on the inlet and outlet columns and
zeros on solid cells, operation for operation as the C writes them. The wall rule cannot be patched in around o.boundaries(): the inlet
and the outlet read f5..f8 of the corner cells after the wall has rewritten them. Everything is fp64, IEEE: strict plans must match it
bit for bit. tests/test_walls_cpu.py pins it, with two no-slip walls, to the unmodified oracle."""
import numpy as np

from oracle.oracle import Oracle, make_params
from tests.reference import Run, feq_rows, link_forces

NOSLIP, FREESLIP = "no-slip", "free-slip"
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]


def moving(u_w):
    return ("moving", float(u_w))


def wall_kind_k(wall):
    """(kind 0 / 1 / 2, k) of a wall given as the binding takes it: k = u_w * (1 / 6), the library's host expression."""
    if wall == NOSLIP:
        return 0, 0.0
    if wall == FREESLIP:
        return 1, 0.0
    name, u_w = wall
    assert name == "moving"
    return 2, float(u_w) * (1.0 / 6.0)


def wall_rule(f, side, kind, k):
    """The table of include/lbm_hip.h (lbm_set_wall) on cells f[..., 9], in place. side 0: south, 1: north."""
    if side == 0:
        f[..., 2] = f[..., 4]
        if kind == 0:
            f[..., 5] = f[..., 7]; f[..., 6] = f[..., 8]
        elif kind == 1:
            f[..., 5] = f[..., 8]; f[..., 6] = f[..., 7]
        else:
            f[..., 5] = f[..., 7] + k; f[..., 6] = f[..., 8] - k
    else:
        f[..., 4] = f[..., 2]
        if kind == 0:
            f[..., 7] = f[..., 5]; f[..., 8] = f[..., 6]
        elif kind == 1:
            f[..., 7] = f[..., 6]; f[..., 8] = f[..., 5]
        else:
            f[..., 7] = f[..., 5] - k; f[..., 8] = f[..., 6] + k
    return f


def boundaries(o, solid, walls, u):
    """lbmo_boundaries in numpy, in its sequential order: bottom, top, inlet, outlet, solid cells. walls = (south, north); u = the inlet
    velocity of every row, [ny]."""
    fc = o.f_current
    ny, nx = solid.shape
    fluid = ~solid
    # the two walls: fluid cells of row 0 / ny - 1 (ghost-inclusive rows 1 / ny)
    for side, gy, y in ((0, 1, 0), (1, ny, ny - 1)):
        kind, k = wall_kind_k(walls[side])
        cols = np.nonzero(fluid[y])[0] + 1
        fc[gy, cols, :] = wall_rule(fc[gy, cols, :], side, kind, k)
    # inlet: fluid cells of column 0, Zou-He velocity with u[y]
    rows = np.nonzero(fluid[:, 0])[0]
    ur = u[rows]
    f = fc[rows + 1, 1, :]
    rho_bc = (f[:, 0] + f[:, 2] + f[:, 4] + 2.0 * (f[:, 3] + f[:, 6] + f[:, 7])) / (1.0 - ur)
    f[:, 1] = f[:, 3] + (2.0 / 3.0) * rho_bc * ur
    f[:, 5] = f[:, 7] - 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho_bc * ur
    f[:, 8] = f[:, 6] + 0.5 * (f[:, 2] - f[:, 4]) + (1.0 / 6.0) * rho_bc * ur
    fc[rows + 1, 1, :] = f
    o.rho[rows, 0] = rho_bc; o.ux[rows, 0] = ur; o.uy[rows, 0] = 0.0
    # outlet: fluid cells of column nx - 1, Zou-He pressure with rho = 1
    rows = np.nonzero(fluid[:, nx - 1])[0]
    f = fc[rows + 1, nx, :]
    rho_out = 1.0
    u_out = -1.0 + (f[:, 0] + f[:, 2] + f[:, 4] + 2.0 * (f[:, 1] + f[:, 5] + f[:, 8])) / rho_out
    f[:, 3] = f[:, 1] - (2.0 / 3.0) * rho_out * u_out
    f[:, 6] = f[:, 8] - 0.5 * (f[:, 2] - f[:, 4]) - (1.0 / 6.0) * rho_out * u_out
    f[:, 7] = f[:, 5] + 0.5 * (f[:, 2] - f[:, 4]) - (1.0 / 6.0) * rho_out * u_out
    fc[rows + 1, nx, :] = f
    o.rho[rows, nx - 1] = rho_out; o.ux[rows, nx - 1] = u_out; o.uy[rows, nx - 1] = 0.0
    # solid cells: the populations reversed, the velocity zeroed
    inner = fc[1:-1, 1:-1]
    inner[solid] = inner[solid][:, OPP]
    o.ux[solid] = 0.0; o.uy[solid] = 0.0


def walls_run(nx, ny, steps, of, *, walls=(NOSLIP, NOSLIP), mask=None, u=None, collide=None, keep_f_current=False, **params):
    """oracle_run of tests/reference.py with `boundaries` above in place of o.boundaries(). walls = (south, north), each "no-slip",
    "free-slip" or ("moving", u_w). Returns a Run (and, with keep_f_current, f_current beside it)."""
    if isinstance(walls, str):
        walls = (walls, walls)
    o = Oracle(make_params(nx, ny, **params))
    if mask is not None:
        o.solid[:] = mask
    o.L.lbmo_initialise(o.h)
    solid = o.solid.astype(bool).copy()
    fluid = ~solid
    if u is not None:                            # interior fluid cells of row y start at f_eq(1, (u[y], 0))
        fr = feq_rows(u)
        for arr in (o.f_current, o.f_next):
            inner = arr[1:-1, 1:-1]
            inner[fluid] = np.broadcast_to(fr[:, None, :], (ny, nx, 9))[fluid]
        o.ux[fluid] = np.broadcast_to(np.asarray(u)[:, None], (ny, nx))[fluid]
        u_rows = np.asarray(u, dtype=np.float64)
    else:
        u_rows = np.full(ny, o.p.inlet_velocity, dtype=np.float64)
    tau = o.p.tau
    forces, bad, tmax = [], -1, None
    for t in range(steps):
        with np.errstate(all="ignore"):          # (a diverging run reaches Inf / NaN; the stability test then ends it)
            got = o.collide() if collide is None else collide(o, tau)
            if got is not None:
                tmax = max(tau if tmax is None else tmax, got)
            if of and t % of == 0:
                forces.append((t,) + link_forces(o.f_next, solid))
            o.exchange_physical()
            o.stream()
            boundaries(o, solid, walls, u_rows)
        if not o.stable():
            bad = t
            break
    out = Run(o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy(), forces, bad, o.solid_count(), tmax)
    fcur = o.f_current.copy()
    o.close()
    return (out, fcur) if keep_f_current else out
