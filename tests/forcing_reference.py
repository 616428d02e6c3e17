"""The reference operator of the uniform driving force (lbm_set_forcing; Guo, Zheng and Shi 2002) for the stepwise oracle loop
(tests/reference.py oracle_run): numpy, fp64, IEEE, in the operation order the library's strict arithmetic evaluates
(lbm_kernels.hpp bgk_collide, the ar_forced phase of the strict branch). Strict plans must match it bit for bit."""
import numpy as np

from tests.reference import CX, CY, PAIRS, W, feq, write_back


def forcing_constants(tau, force):
    """(wp, gx, gy, hx, hy) as the host forms them in double: wp = 1/tau, g = (1 - wp/2) F, h = F/2."""
    fx, fy = float(force[0]), float(force[1])
    wp = 1.0 / tau
    k = 1.0 - 0.5 * wp
    return wp, k * fx, k * fy, 0.5 * fx, 0.5 * fy


def guo_source(r, ux, uy, gx, gy):
    """The nine source terms S_i = w_i ((3 cg - u3) + (9 cu) cg), u3 = 3 (ux gx + uy gy), with cu and cg per opposite pair; the
    opposite direction negates 3 cg and keeps the product. gx, gy: the host's doubles, cast once to the cells' element type, in which
    gx + gy and gx - gy of the diagonal pairs are formed (lbm_kernels.hpp bgk_collide, the ar_forced phase: both are T there)."""
    gx, gy = r.dtype.type(gx), r.dtype.type(gy)
    u3 = 3.0 * (ux * gx + uy * gy)
    s = [None] * 9
    s[0] = W[0] * (0.0 - u3)
    for (i, ib), cu, cg in zip(PAIRS, (ux, uy, ux + uy, ux - uy), (gx, gy, gx + gy, gx - gy)):
        a = 3.0 * cg
        b = (9.0 * cu) * cg
        s[i] = W[i] * ((a - u3) + b)
        s[ib] = W[i] * (((-a) - u3) + b)
    return s


def guo_moments(o, hx, hy):
    """tests/reference.py `moments` with h added to the momenta before the two divisions (it divides inside: restated)."""
    fluid = ~o.solid.astype(bool)
    f = [o.f_current[1:-1, 1:-1, i][fluid] for i in range(9)]
    r = np.zeros_like(f[0]); jx = np.zeros_like(f[0]); jy = np.zeros_like(f[0])
    for i in range(9):
        r = r + f[i]
        jx = jx + float(CX[i]) * f[i]
        jy = jy + float(CY[i]) * f[i]
    jx = jx + hx
    jy = jy + hy
    return fluid, f, r, jx / r, jy / r


def guo_collide(o, tau, force):
    """lbmo_collide under the force density `force` = (Fx, Fy): the equilibrium at u = (sum c f + F/2) / rho, relaxed with 1/tau as
    BGK relaxes, plus the source. Writes back rho and Guo's ux, uy."""
    wp, gx, gy, hx, hy = forcing_constants(tau, force)
    fluid, f, r, ux, uy = guo_moments(o, hx, hy)
    usq = ux * ux + uy * uy
    s = guo_source(r, ux, uy, gx, gy)
    out = [(f[i] - wp * (f[i] - feq(i, r, ux, uy, usq))) + s[i] for i in range(9)]
    write_back(o, fluid, out, r, ux, uy)
