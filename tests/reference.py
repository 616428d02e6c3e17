"""The one stepwise reference run of the GPU feature tests (test infrastructure, like oracle/oracle.py).

The C oracle's arrays are writable views, so its loop taken step by step, with a numpy collision operator in place of o.collide()
and a numpy restatement of ALL of lbmo_boundaries (oracle/lbm_oracle.c) in place of o.boundaries(), is the reference of every feature
the oracle itself does not have: obstacle masks, inlet profiles and schedules, the wall kinds, the collision operators, and any
combination of them. Everything here is IEEE, in the operation order the library's strict arithmetic evaluates: strict plans must
match it bit for bit. tests/test_reference_cpu.py pins the loop and the shared pieces to the unmodified oracle.

dtype=np.float64 (the default) runs on the C oracle. dtype=np.float32 runs the same loop on tests/numpy_oracle.py NumpyOracle, whose
arrays are float32: every operation below is then one IEEE float32 operation, a Python float that meets an array is rounded to float32
first (the library's T(constant), or its host value formed in double and cast once), and what the library forms in the element type
on the device (the inlet velocity of a row times the schedule's factor, g_x + g_y of the driving force) is formed from float32 values
here. The strict fp32 plans must match such a run bit for bit (tests/test_gpu_f32_oracle.py); tests/test_f32_reference_cpu.py pins
NumpyOracle in float64 to the C oracle."""
import collections
import math

import numpy as np

from oracle.oracle import Oracle, make_params
from tests.numpy_oracle import NumpyOracle

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
    """f_next on the interior's fluid cells, and rho / ux / uy recorded as the oracle does. (An assignment into the oracle's arrays
    would cast silently: an operator that left the oracle's element type on the way is stopped here.)"""
    assert all(v.dtype == o.f_next.dtype for v in list(out) + [r, vx, vy]), "the collision operator left " + str(o.f_next.dtype)
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
        s = float(np.sum(f[..., i][sel].astype(np.float64)))      # (k_forces widens each population and sums in double)
        fx += 2.0 * CX[i] * s
        fy += 2.0 * CY[i] * s
    return fx, fy


# ---- the boundary step: walls, inlet, outlet, solid cells -----------------------------------------------------------------------
NOSLIP, FREESLIP = "no-slip", "free-slip"
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]
HOLD, REPEAT = 0, 1


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


def sched_index(t, n, mode):
    """Which entry iteration t takes: HOLD s[min(t, n - 1)], REPEAT s[t mod n] (the Python restatement of inlet_sched_index)."""
    return t % n if mode == REPEAT else min(t, n - 1)


def boundaries(o, solid, walls, u):
    """lbmo_boundaries in numpy, in its sequential order: bottom, top, inlet, outlet, solid cells, with rho / ux / uy on the inlet and
    outlet columns and zeros on solid cells, operation for operation as the C writes them. walls = (south, north); u = the inlet
    velocity of every row, [ny]. (A wall rule cannot be patched in around o.boundaries(): the inlet and the outlet read f5..f8 of the
    corner cells after the wall has rewritten them.)"""
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
    assert rho_bc.dtype == ur.dtype == fc.dtype, "the inlet left " + str(fc.dtype)      # (the assignments would cast silently)
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


# ---- the loop -------------------------------------------------------------------------------------------------------------------
Run = collections.namedtuple("Run", "f_next rho ux uy forces first_unstable solid_count tau_max solid forced", defaults=(None, None))


def open_run(nx, ny, dtype, backend, mask, u, schedule, **params):
    """What the reference loops (oracle_run, ports_run, periodic_run) share in front of their iterations: the oracle on `mask` in its
    initial state, and the inlet. Returns (o, solid, u_at): o the C oracle (dtype float64) or a NumpyOracle (any other dtype; backend
    "numpy": float64 too); u_at(t) the inlet velocity of every row at iteration t, in dtype.
    As the library forms them: the profile and the schedule's factors are each cast to dtype (upload_rows, upload_schedule) and their
    product is ONE multiplication in dtype (lbm_kernels.hpp bcs_at_with, macro_cell); the initial state under a profile or a schedule
    is f_eq(1, (u[y] * s[0], 0)) with the product and the equilibrium formed in double and cast once (prepare_schedule, upload_feqrow)."""
    dtype = np.dtype(dtype)
    p = make_params(nx, ny, **params)
    o = Oracle(p) if (dtype == np.float64 and backend != "numpy") else NumpyOracle(p, dtype)
    if mask is not None:
        o.solid[:] = mask
    o.initialise()
    solid = o.solid.astype(bool).copy()
    fluid = ~solid
    u_rows = np.full(ny, o.p.inlet_velocity, dtype=np.float64) if u is None else np.asarray(u, dtype=np.float64)
    s, mode = (None, HOLD) if schedule is None else (np.asarray(schedule[0], dtype=np.float64), schedule[1])
    if u is not None or s is not None:           # interior fluid cells of row y start at f_eq(1, (u0[y], 0))
        u0 = u_rows if s is None else u_rows * s[0]
        fr = feq_rows(u0)
        for arr in (o.f_current, o.f_next):
            inner = arr[1:-1, 1:-1]
            inner[fluid] = np.broadcast_to(fr[:, None, :], (ny, nx, 9))[fluid]
        o.ux[fluid] = np.broadcast_to(u0[:, None], (ny, nx))[fluid]
    u_t = u_rows.astype(dtype)
    s_t = None if s is None else s.astype(dtype)

    def u_at(t):
        return u_t if s_t is None else u_t * s_t[sched_index(t, len(s_t), mode)]
    return o, solid, u_at


def close_run(o, solid, forces, bad, tmax, collide, keep_f_current):
    """The Run of a finished loop (and, with keep_f_current, f_current beside it); closes the oracle."""
    force = getattr(collide, "keywords", {}).get("force")           # (a guo_collide partial: what `snapshot` takes off the momentum)
    out = Run(o.f_next.copy(), o.rho.copy(), o.ux.copy(), o.uy.copy(), forces, bad, o.solid_count(), tmax, solid, force)
    fcur = o.f_current.copy()
    o.close()
    return (out, fcur) if keep_f_current else out


def oracle_run(nx, ny, steps, of, *, mask=None, u=None, walls=(NOSLIP, NOSLIP), schedule=None, collide=None, keep_f_current=False,
               dtype=np.float64, backend=None, **params):
    """The stepwise oracle: on `mask` (None: the analytic disc of `params`); with the inlet of row y at iteration t at u[y] (None: the
    uniform inlet_velocity of `params`) times, under schedule = (s, HOLD or REPEAT), s[sched_index(t)] — one IEEE multiplication in
    dtype, formed before `boundaries` uses it; between walls = (south, north), each "no-slip", "free-slip" or ("moving", u_w), one
    string meaning both; and with collide(o, tau) in place of its own o.collide() (None: plain BGK). forces are [(t, fx, fy)] by
    link_forces; tau_max is the largest value the operator returned, None if it returns none. dtype, backend: see open_run. Returns a
    Run (and, with keep_f_current, f_current beside it)."""
    if isinstance(walls, str):
        walls = (walls, walls)
    o, solid, u_at = open_run(nx, ny, dtype, backend, mask, u, schedule, **params)
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
            boundaries(o, solid, walls, u_at(t))
        if not o.stable():
            bad = t
            break
    return close_run(o, solid, forces, bad, tmax, collide, keep_f_current)


# ---- the macro snapshot ----------------------------------------------------------------------------------------------------------
def snapshot(run):
    """(rho, ux, uy) of ctx.macros() after the run's iterations, restated from the run's arrays in the run's dtype (lbm_kernels.hpp
    macro_cell; csrc/lbm_steps.inc.hpp do_macros: it reads the buffer the last step kernel READ, which is the run's f_next, and
    describes the run's last iteration):
      * a fluid cell off the two port columns: the moments of its nine populations of f_next in the element type, i ascending, then
        the two divisions; under a driving force h = F/2, cast once, is taken off each momentum before its division (macro_moments);
      * a fluid cell of column 0 or nx - 1: (rho, u, 0) of the port's rule on the populations pulled from f_next behind the wall rule,
        which is what `boundaries` recorded in rho / ux / uy at the last iteration, operation for operation: taken from there;
      * a solid cell: (1, 0, 0), which rho / ux / uy hold too.
    The oracle's rho / ux / uy of the other fluid cells are moments of f_current, another set of populations with the same sums up to
    rounding: close to the snapshot, not equal to it."""
    assert run.first_unstable == -1 and run.solid is not None
    rho, ux, uy = run.rho.copy(), run.ux.copy(), run.uy.copy()
    ny, nx = run.solid.shape
    if nx > 2:
        sel = ~run.solid[:, 1:-1]
        f = [run.f_next[1:-1, 2:-2, i][sel] for i in range(9)]
        r = np.zeros_like(f[0]); sx = np.zeros_like(f[0]); sy = np.zeros_like(f[0])
        for i in range(9):
            r = r + f[i]
            sx = sx + float(CX[i]) * f[i]
            sy = sy + float(CY[i]) * f[i]
        if run.forced is not None:
            sx = sx - 0.5 * float(run.forced[0])
            sy = sy - 0.5 * float(run.forced[1])
        for a, v in ((rho, r), (ux, sx / r), (uy, sy / r)):
            inner = a[:, 1:-1]
            inner[sel] = v
    return rho, ux, uy
