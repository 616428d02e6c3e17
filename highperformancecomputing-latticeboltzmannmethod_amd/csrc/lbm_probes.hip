// csrc/lbm_probes.hip — k_probes: one sample of every point probe (rho, ux, uy; lbm_probes.hpp) from the populations P_t, for both
// element types. A translation unit of its own (build.py): it compiles beside lbm_hip.hip and leaves every step kernel untouched.
//
// One launch per sample whatever n: 256-thread blocks, one thread per probe. The thread reads its table entry, calls macro_cell for the
// one to four cells of nonzero weight (nine populations each; the inlet and outlet columns pull + wall + Zou-He as k_macros does),
// interpolates in double and stores three doubles into the ring slot — or three +0.0 where another strip owns the probe. No LDS, no
// atomics, plain vector stores. The loads are scattered (a probe is a point); at n = 65536 the kernel reads at most 4 x 9 populations
// per probe, 19 MB at fp64, and writes 1.5 MB.
// No contraction: every product and sum below is rounded to double (the pragma), and the inlined macro_cell relies on the object's
// -ffp-contract=off as it does inside k_stats, so the cells' macros are those of k_macros to the bit.
#include "lbm_probes.hpp"

namespace lbmk {

template <typename T>
__global__ void __launch_bounds__(PROBE_THREADS) k_probes(const ProbeArgs<T> p) {
#pragma clang fp contract(off)
    const int j = (int)(blockIdx.x * PROBE_THREADS + threadIdx.x);
    if (j >= p.n) return;
    const MacroArgs<T>& a = p.m;
    const ProbeEntry e = p.table[j];
    double r = 0.0, vx = 0.0, vy = 0.0;
    if (e.owned) {
        const int x0 = e.x0, y0 = e.y0;
        const int x1 = x0 + 1 < a.nx ? x0 + 1 : a.nx - 1;
        const int y1 = a.y_start + y0 + 1 < a.ny_glob ? y0 + 1 : y0;      // (local: ny_loc is the ghost row next to the north face)
        const double fx = e.fx, fy = e.fy;
        macro_cell<T>(a, x0, y0, r, vx, vy);
        if (fx != 0.0) {
            double r1, vx1, vy1;
            macro_cell<T>(a, x1, y0, r1, vx1, vy1);
            const double gx = 1.0 - fx;
            r = gx * r + fx * r1; vx = gx * vx + fx * vx1; vy = gx * vy + fx * vy1;
        }
        if (fy != 0.0) {
            double rb, vxb, vyb;
            macro_cell<T>(a, x0, y1, rb, vxb, vyb);
            if (fx != 0.0) {
                double r1, vx1, vy1;
                macro_cell<T>(a, x1, y1, r1, vx1, vy1);
                const double gx = 1.0 - fx;
                rb = gx * rb + fx * r1; vxb = gx * vxb + fx * vx1; vyb = gx * vyb + fx * vy1;
            }
            const double gy = 1.0 - fy;
            r = gy * r + fy * rb; vx = gy * vx + fy * vxb; vy = gy * vy + fy * vyb;
        }
    }
    double* o = p.out + 3L * j;
    o[0] = r; o[1] = vx; o[2] = vy;
}

template <typename T>
void launch_probes(const ProbeArgs<T>& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n + PROBE_THREADS - 1) / PROBE_THREADS)), block(PROBE_THREADS);
    hipLaunchKernelGGL((k_probes<T>), grid, block, 0, s, a);
}

template void launch_probes<double>(const ProbeArgs<double>&, hipStream_t);
template void launch_probes<float>(const ProbeArgs<float>&, hipStream_t);

}  // namespace lbmk
