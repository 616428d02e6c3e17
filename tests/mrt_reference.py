"""The reference of the MRT collision (lbm_set_mrt; test infrastructure, like tests/reference.py): numpy, fp64, IEEE, in the operation
order the library's strict arithmetic evaluates (include/lbm_hip.h lbm_set_mrt; csrc/lbm_kernels.hpp bgk_collide, the ar_mrt branch of
`pair`), so that strict plans must match it bit for bit. Passed as collide= to the reference loops (oracle_run and the ports, periodic
and forcing loops)."""
import functools
import importlib

import numpy as np

from tests.helpers import PKG, square
from tests.reference import feq, moments, oracle_run, trt_collide, write_back

GROUPS = [((1, 3), (2, 4)), ((5, 7), (8, 6))]         # the axis pairs, the diagonal pairs


def mrt_rates(tau, bulk_rate, magic):
    """(sb, wp, wm) as the host forms them in double."""
    return float(bulk_rate), 1.0 / tau, 1.0 / (0.5 + magic / (tau - 0.5))


def mrt_cells(f, r, vx, vy, tau, bulk_rate, magic):
    """The operator on bare cells: f the list of nine arrays, r / vx / vy their density and velocity. Returns the nine relaxed arrays."""
    sb, wp, wm = mrt_rates(tau, bulk_rate, magic)
    usq = vx * vx + vy * vy
    fe = [feq(i, r, vx, vy, usq) for i in range(9)]
    out = [None] * 9
    out[0] = f[0] - sb * (f[0] - fe[0])
    for (i, ib), (j, jb) in GROUPS:
        np_p = 0.5 * ((f[i] + f[ib]) - (fe[i] + fe[ib]))
        nm_p = 0.5 * ((f[i] - f[ib]) - (fe[i] - fe[ib]))
        o_p = wm * nm_p
        np_q = 0.5 * ((f[j] + f[jb]) - (fe[j] + fe[jb]))
        nm_q = 0.5 * ((f[j] - f[jb]) - (fe[j] - fe[jb]))
        o_q = wm * nm_q
        t = 0.5 * (np_p + np_q)
        d = 0.5 * (np_p - np_q)
        a = sb * t
        b = wp * d
        e_p = a + b
        e_q = a - b
        out[i] = (f[i] - e_p) - o_p
        out[ib] = (f[ib] - e_p) + o_p
        out[j] = (f[j] - e_q) - o_q
        out[jb] = (f[jb] - e_q) + o_q
    return out


def mrt_collide(o, tau, bulk_rate, magic):
    """lbmo_collide with the MRT operator: TRT's even and odd parts of each opposite pair; the half sum of the even parts of the two
    axis pairs (and of the two diagonal pairs) and the rest population relax with the bulk rate, the half difference with 1/tau, the
    odd parts with wm = 1/(0.5 + magic/(tau - 0.5))."""
    fluid, f, r, vx, vy = moments(o)
    write_back(o, fluid, mrt_cells(f, r, vx, vy, tau, bulk_rate, magic), r, vx, vy)


# ---- the cases of the plan-against-reference tests (tests/test_mrt_cpu.py, tests/test_gpu_mrt.py): computed once, shared, read-only ----
NX, NY, STEPS, OF = 160, 48, 240, 60
BULK, MAGIC = 1.0, 3.0 / 16.0
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)
CASES = ["disc", "square", "disc-parabolic"]


def case_inputs(name):
    lbm = importlib.import_module(PKG)
    mask = square(NX, NY) if name == "square" else None
    u = lbm.parabolic_profile(NY, KW["inlet_velocity"]) if name == "disc-parabolic" else None
    return mask, u


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the MRT reference run, max |f_mrt - f_trt| against TRT with the same magic parameter on the same case)."""
    mask, u = case_inputs(name)
    ref = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, collide=functools.partial(mrt_collide, bulk_rate=BULK, magic=MAGIC), **KW)
    trt = oracle_run(NX, NY, STEPS, OF, mask=mask, u=u, collide=functools.partial(trt_collide, magic=MAGIC), **KW)
    for a in (ref.f_next, ref.rho, ref.ux, ref.uy):
        a.flags.writeable = False
    return ref, float(np.max(np.abs(ref.f_next - trt.f_next)))
