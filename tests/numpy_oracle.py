"""oracle/lbm_oracle.c restated in numpy for any element type (test infrastructure, like oracle/oracle.py).

NumpyOracle(params, dtype) offers the part of oracle.oracle.Oracle that the reference loops use (tests/reference.py oracle_run,
tests/ports_reference.py ports_run, tests/periodic_reference.py periodic_run), operation for operation as the C writes it: the disc by
solid_global, the ghost-inclusive arrays, the E/W ghost columns zeroed by exchange_physical, the N/S ghost rows left at their initial
values, the stability scan over ghost and solid cells too. In float64 it is the C oracle to the bit (tests/test_f32_reference_cpu.py).
In float32 every array is float32 and every operation one IEEE float32 operation: a Python float that meets a float32 array is rounded
to float32 first, which is the library's T(constant), and a host value "formed in double and cast once" is a Python float expression
used once. That is what the library's strict fp32 kernels evaluate, so they must match a float32 run bit for bit.

Where float32 makes a difference the library decides, not the C oracle:
  * the initial state is feq_inflow evaluated in double and cast once (csrc/lbm_hip.hip feq_inflow, upload_feqrow, upload_rows);
  * 1/tau is formed in double and cast once (csrc/lbm_launch.inc.hpp make_kargs)."""
import numpy as np

CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]
W = [4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4


def feq_init(rho, ux, uy):
    """lbm_oracle.c feq_init on Python floats, that is in double: the bracket ((1 + 3cu) - 1.5u^2) + 4.5cu^2, then (w rho) * bracket."""
    usq = ux * ux + uy * uy
    f = [W[0] * rho * (1.0 - 1.5 * usq)]
    t3 = 1.5 * usq
    for i in range(1, 9):
        cu = float(CX[i]) * ux + float(CY[i]) * uy
        br = ((1.0 + 3.0 * cu) - t3) + 4.5 * (cu * cu)
        f.append((W[i] * rho) * br)
    return f


class NumpyOracle:
    """One whole domain of the restatement. params: oracle.make_params(...); dtype: np.float64 or np.float32."""

    def __init__(self, params, dtype=np.float64):
        self.p = params
        self.dtype = np.dtype(dtype)
        self.nx, self.ny = params.nx, params.ny
        self.local_ny = self.ny
        nx, ny = self.nx, self.ny
        # lbmo_cylinder_*_cells, solid_global: integer cells, dx*dx + dy*dy <= r*r (exact in double, so in integers)
        cx, cy, r = int(params.cylinder_x * nx), int(params.cylinder_y * ny), int(params.cylinder_radius * ny)
        y, x = np.mgrid[0:ny, 0:nx]
        self.solid = (((x - cx) ** 2 + (y - cy) ** 2) <= r * r).astype(np.uint8)
        self.initialise()

    def close(self):
        pass

    def initialise(self):
        """lbmo_initialise: every cell of both arrays, ghosts included, at f_eq(1, (u_in, 0)); solid cells at f_eq(1, 0)."""
        nx, ny, T = self.nx, self.ny, self.dtype
        fe = np.array(feq_init(1.0, float(self.p.inlet_velocity), 0.0), dtype=np.float64).astype(T)
        fs = np.array(feq_init(1.0, 0.0, 0.0), dtype=np.float64).astype(T)
        s = self.solid.astype(bool)
        self.f_current = np.empty((ny + 2, nx + 2, 9), T)
        self.f_current[:] = fe
        self.f_current[1:-1, 1:-1][s] = fs
        self.f_next = self.f_current.copy()
        self.rho = np.ones((ny, nx), T)
        self.uy = np.zeros((ny, nx), T)
        self.ux = np.where(s, 0.0, float(self.p.inlet_velocity)).astype(T)

    def solid_count(self):
        return int(np.sum(self.solid != 0))

    def collide(self):
        """lbmo_collide: plain BGK on the interior's fluid cells."""
        tau_inv = 1.0 / self.p.tau
        fluid = ~self.solid.astype(bool)
        f = [self.f_current[1:-1, 1:-1, i][fluid] for i in range(9)]
        r = np.zeros_like(f[0]); vx = np.zeros_like(f[0]); vy = np.zeros_like(f[0])
        for i in range(9):
            r = r + f[i]
            vx = vx + float(CX[i]) * f[i]
            vy = vy + float(CY[i]) * f[i]
        vx = vx / r
        vy = vy / r
        self.rho[fluid] = r; self.ux[fluid] = vx; self.uy[fluid] = vy
        usq = vx * vx + vy * vy
        inner = self.f_next[1:-1, 1:-1]
        for i in range(9):
            cu = float(CX[i]) * vx + float(CY[i]) * vy
            feq = W[i] * r * (1.0 + 3.0 * cu + 4.5 * cu * cu - 1.5 * usq)
            col = inner[:, :, i]
            col[fluid] = f[i] - tau_inv * (f[i] - feq)

    def exchange_physical(self):
        """lbmo_exchange_physical: the E/W ghost columns of f_next, rows 1 .. ny, become zero; the N/S ghost rows are not touched."""
        self.f_next[1:-1, 0, :] = 0.0
        self.f_next[1:-1, -1, :] = 0.0

    def edge_row(self, north):
        """lbmo_get_edge_row: the north / south interior edge row of f_next, nx * 9 values."""
        return self.f_next[self.ny if north else 1, 1:-1, :].reshape(-1).copy()

    def set_ghost_row(self, north, buf):
        """lbmo_set_ghost_row: into the north / south ghost row of f_next, its two end cells zero."""
        gy = self.ny + 1 if north else 0
        self.f_next[gy, 1:-1, :] = np.asarray(buf).reshape(self.nx, 9)
        self.f_next[gy, 0, :] = 0.0
        self.f_next[gy, -1, :] = 0.0

    def stream(self):
        """lbmo_stream: f_current(x, i) = f_next(x - c_i, i) on the interior."""
        ny, nx = self.ny, self.nx
        for i in range(9):
            self.f_current[1:-1, 1:-1, i] = self.f_next[1 - CY[i]:1 - CY[i] + ny, 1 - CX[i]:1 - CX[i] + nx, i]

    def stable(self):
        """lbmo_check_stability over all of f_current: NaN, > 1e5, < -1e5 flag the run; the last (total mod 4) values also at |v| = 1e5
        (1e5 is exact in float32 too)."""
        v = self.f_current.reshape(-1)
        end = (v.size // 4) * 4
        head, tail = v[:end], v[end:]
        with np.errstate(invalid="ignore"):
            if np.any((head != head) | (head > 1e5) | (head < -1e5)):
                return False
            return bool(np.all(np.isfinite(tail) & (np.abs(tail) < 1e5)))
