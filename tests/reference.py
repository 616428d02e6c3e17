"""The one stepwise reference run of the GPU feature tests (test infrastructure, like oracle/oracle.py).

The C oracle's arrays are writable views, so its loop taken step by step, with a numpy collision operator in place of o.collide()
and a numpy fix-up of the inlet column, is the reference of every feature the oracle itself does not have. Everything here is fp64,
IEEE, in the operation order the library's strict arithmetic evaluates: strict plans must match it bit for bit.
tests/test_reference_cpu.py pins the shared pieces to the unmodified oracle."""
import collections
import math

import numpy as np

from oracle.oracle import Oracle, make_params

CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]
W = [4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4
PAIRS = [(1, 3), (2, 4), (5, 7), (8, 6)]


# ---- moments, equilibrium and write-back shared by the collision operators -----------------------------------------------------
def moments(o):
    """(fluid, f, rho, ux, uy) of the interior's fluid cells as lbmo_collide forms them (lbm_oracle.c): r += f_i; vx += cx_i f_i;
    vy += cy_i f_i, i ascending, then the two divisions."""
    fluid = ~o.solid.astype(bool)
    f = [o.f_current[1:-1, 1:-1, i][fluid] for i in range(9)]
    r = np.zeros_like(f[0]); vx = np.zeros_like(f[0]); vy = np.zeros_like(f[0])
    for i in range(9):
        r = r + f[i]
        vx = vx + float(CX[i]) * f[i]
        vy = vy + float(CY[i]) * f[i]
    return fluid, f, r, vx / r, vy / r


def feq(i, r, vx, vy, usq):
    """The collision's equilibrium (not feq_init's order: see feq_rows)."""
    cu = float(CX[i]) * vx + float(CY[i]) * vy
    return W[i] * r * (((1.0 + 3.0 * cu) + (4.5 * cu) * cu) - 1.5 * usq)


def write_back(o, fluid, out, r, vx, vy):
    """f_next on the interior's fluid cells, and rho / ux / uy recorded as the oracle does."""
    inner = o.f_next[1:-1, 1:-1]
    for i in range(9):
        col = inner[:, :, i]
        col[fluid] = out[i]
        inner[:, :, i] = col
    o.rho[fluid] = r
    o.ux[fluid] = vx
    o.uy[fluid] = vy


# ---- collision operators: collide(o, tau) ---------------------------------------------------------------------------------------
def les_collide(o, tau, cs):
    """lbmo_collide with the Smagorinsky relaxation time of each fluid cell (lbm_kernels.hpp les_tau_inv_strict):
    f_next = f - (1/tau_eff)(f - feq). Returns the largest tau_eff."""
    tau2, c = tau * tau, 18.0 * math.sqrt(2.0) * (cs * cs)
    fluid, f, r, vx, vy = moments(o)
    sxx = ((((f[1] + f[3]) + f[5]) + f[6]) + f[7]) + f[8]
    syy = ((((f[2] + f[4]) + f[5]) + f[6]) + f[7]) + f[8]
    sxy = ((f[5] - f[6]) + f[7]) - f[8]
    pxx = (sxx - r * (vx * vx)) - r * (1.0 / 3.0)
    pyy = (syy - r * (vy * vy)) - r * (1.0 / 3.0)
    pxy = sxy - r * (vx * vy)
    qn = np.sqrt((pxx * pxx + pyy * pyy) + 2.0 * (pxy * pxy))
    tau_eff = 0.5 * (tau + np.sqrt(tau2 + c * (qn / r)))
    tinv = 1.0 / tau_eff
    usq = vx * vx + vy * vy
    write_back(o, fluid, [f[i] - tinv * (f[i] - feq(i, r, vx, vy, usq)) for i in range(9)], r, vx, vy)
    return float(np.max(tau_eff)) if tau_eff.size else tau


def trt_collide(o, tau, magic):
    """lbmo_collide with the two-relaxation-time operator (lbm_kernels.hpp bgk_collide, the ar_trt branch of `pair`): the rest
    population relaxed with wp = 1/tau, each opposite pair split into its even and odd non-equilibrium parts, relaxed with wp and
    wm = 1/(0.5 + magic/(tau - 0.5))."""
    wp = 1.0 / tau
    wm = 1.0 / (0.5 + magic / (tau - 0.5))
    fluid, f, r, vx, vy = moments(o)
    usq = vx * vx + vy * vy
    fe = [feq(i, r, vx, vy, usq) for i in range(9)]
    out = [None] * 9
    out[0] = f[0] - wp * (f[0] - fe[0])
    for i, ib in PAIRS:
        n_p = 0.5 * ((f[i] + f[ib]) - (fe[i] + fe[ib]))
        n_m = 0.5 * ((f[i] - f[ib]) - (fe[i] - fe[ib]))
        out[i] = (f[i] - wp * n_p) - wm * n_m
        out[ib] = (f[ib] - wp * n_p) + wm * n_m
    write_back(o, fluid, out, r, vx, vy)


# ---- the inlet profile and the forces -------------------------------------------------------------------------------------------
def feq_rows(u):
    """f_eq(1, (u[y], 0)) per row in the oracle's feq_init order (lbm_oracle.c), which is not the collision's: [ny, 9]."""
    u = np.asarray(u, dtype=np.float64)[:, None]
    cx, cy, w = (np.array(v, dtype=np.float64)[None, :] for v in (CX, CY, W))
    uy = 0.0
    usq = u * u + uy * uy
    t3 = 1.5 * usq
    cu = cx * u + cy * uy
    f = (w * 1.0) * (((1.0 + 3.0 * cu) - t3) + 4.5 * (cu * cu))
    f[:, 0] = (W[0] * 1.0 * (1.0 - 1.5 * usq))[:, 0]
    return f


def link_forces(f_next, solid):
    """IOManager::record_forces (LBMIO.h:133-160; oracle/lbm_oracle.c lbmo_forces): every solid cell, every direction i whose
    fluid end x - c_i lies in the domain: F += 2 c_i f_i(x - c_i) on the post-collision populations (ghost-inclusive array)."""
    ny, nx = solid.shape
    fx = fy = 0.0
    f = f_next[1:-1, 1:-1]
    for i in range(1, 9):
        # fluid cell (x, y) whose neighbour (x + cx, y + cy) is solid
        nb = np.zeros_like(solid)
        ys, yd = (slice(CY[i], None), slice(0, ny - CY[i])) if CY[i] >= 0 else (slice(0, ny + CY[i]), slice(-CY[i], None))
        xs, xd = (slice(CX[i], None), slice(0, nx - CX[i])) if CX[i] >= 0 else (slice(0, nx + CX[i]), slice(-CX[i], None))
        nb[yd, xd] = solid[ys, xs]
        sel = nb & ~solid
        s = float(np.sum(f[..., i][sel]))
        fx += 2.0 * CX[i] * s
        fy += 2.0 * CY[i] * s
    return fx, fy


# ---- the loop -------------------------------------------------------------------------------------------------------------------
Run = collections.namedtuple("Run", "f_next rho ux uy forces first_unstable solid_count tau_max")


def oracle_run(nx, ny, steps, of, *, mask=None, u=None, collide=None, **params):
    """The stepwise oracle: on `mask` (None: the analytic disc of `params`), with the inlet of row y at u[y] (None: the uniform
    inlet) and with collide(o, tau) in place of its own o.collide() (None: plain BGK). forces are [(t, fx, fy)] by link_forces;
    tau_max is the largest value the operator returned, None if it returns none."""
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
        rows = np.nonzero(fluid[:, 0])[0]
        ur = np.asarray(u, dtype=np.float64)[rows]
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
        o.boundaries()
        if u is not None:
            # the inlet again, with u[y]: it reads f0, f2, f3, f4, f6, f7 after the wall conditions (which it leaves alone) and
            # rewrites f1, f5, f8 (lbm_oracle.c inlet block, same operation order)
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
    out = Run(o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy(), forces, bad, o.solid_count(), tmax)
    o.close()
    return out
