"""The reference of the outlet sponge (lbm_set_sponge; test infrastructure, like tests/reference.py): numpy, IEEE, in the operation
order the library's strict arithmetic evaluates (include/lbm_hip.h lbm_set_sponge; csrc/lbm_kernels.hpp bgk_collide with the rate of
the cell's column), so that strict plans must match it bit for bit in the oracle's dtype. Passed as collide= to the reference loops
(oracle_run, ports_run, periodic_run)."""
import functools
import importlib

import numpy as np

from tests.helpers import PKG
from tests.reference import feq, moments, oracle_run, write_back


def sponge_rates(nx, tau, width, tau_end, dtype):
    """The table the kernels read: 1 / sponge_tau of every column, formed in double, cast once to dtype."""
    lbm = importlib.import_module(PKG)
    return (1.0 / lbm.sponge_tau(nx, tau, width, tau_end)).astype(dtype)


def sponge_collide(o, tau, width, tau_end):
    """lbmo_collide with the rate of the cell's column in place of 1/tau: f_i - wp_x (f_i - feq_i), operation by operation as BGK."""
    fluid, f, r, vx, vy = moments(o)
    ny, nx = fluid.shape
    wp = np.broadcast_to(sponge_rates(nx, tau, width, tau_end, o.f_next.dtype)[None, :], (ny, nx))[fluid]
    usq = vx * vx + vy * vy
    write_back(o, fluid, [f[i] - wp * (f[i] - feq(i, r, vx, vy, usq)) for i in range(9)], r, vx, vy)


# ---- the cases of the plan-against-reference tests (tests/test_sponge_cpu.py, tests/test_gpu_sponge.py): computed once, shared, read-only
NX, NY, STEPS, OF = 160, 48, 240, 60
WIDTH, TAU_END = 48, 1.5
SPONGE = (WIDTH, TAU_END)
KW = dict(tau=0.55, inlet_velocity=0.08, cylinder_radius=0.1)


def collide_of(width=WIDTH, tau_end=TAU_END):
    return functools.partial(sponge_collide, width=width, tau_end=tau_end)


def read_only(run):
    for a in (run.f_next, run.rho, run.ux, run.uy, run.solid):
        a.flags.writeable = False
    return run


@functools.lru_cache(maxsize=None)
def reference(precision="f64", sponge=True):
    """The reference run of the disc case in "f64" or "f32", with the sponge or (sponge=False) plain BGK."""
    dtype = {"f32": np.float32, "f64": np.float64}[precision]
    return read_only(oracle_run(NX, NY, STEPS, OF, collide=collide_of() if sponge else None, dtype=dtype, **KW))


@functools.lru_cache(maxsize=None)
def edge_reference(nx, ny, width, steps, of):
    """The fp64 reference of an edge shape of tests/test_gpu_sponge.py: the disc case's physics on another lattice and zone."""
    return read_only(oracle_run(nx, ny, steps, of, collide=collide_of(width, TAU_END), **KW))


# ---- what comes back from the outlet (tests/test_sponge_cpu.py; profiles/sponge/README.md) --------------------------------------------
R_NX, R_NY, R_W, R_TAU_END, R_STEPS = 200, 40, 48, 1.5, 700
R_KW = dict(tau=0.53, inlet_velocity=0.08, cylinder_radius=0.1)
R_COLS = slice(60, 120)


def density_ripple(run):
    """The largest |rho - mean| over columns 60..119 of the run's last iteration: the pressure wave of the impulsive start, which by
    iteration 700 has crossed the channel, met the outlet and come back into these columns."""
    rho = run.rho[:, R_COLS]
    sel = ~run.solid[:, R_COLS]
    return float(np.max(np.abs(rho[sel] - np.mean(rho[sel]))))


@functools.lru_cache(maxsize=None)
def reflection_pair():
    """(plain BGK's ripple, the sponge's ripple) of the 200x40 case after 700 iterations."""
    plain = oracle_run(R_NX, R_NY, R_STEPS, 0, **R_KW)
    sponge = oracle_run(R_NX, R_NY, R_STEPS, 0, collide=collide_of(R_W, R_TAU_END), **R_KW)
    assert plain.first_unstable == sponge.first_unstable == -1
    return density_ripple(plain), density_ripple(sponge)
