// csrc/lbm_probes.hpp — what the host translation unit (lbm_hip.hip) sees of the probe kernel (lbm_probes_begin; the reference has
// none): the table entry of a probe, the one function that derives it, the kernel's arguments and one launcher per element type. The
// kernel itself is compiled in its own translation unit (lbm_probes.hip), beside the others (build.py).
//
// A PROBE is a point (px, py) in global lattice coordinates, 0 <= px <= nx - 1, 0 <= py <= ny - 1. Its SAMPLE of iteration t is
// (rho, ux, uy) in double, interpolated bilinearly from the snapshot macro_cell defines (lbm_kernels.hpp), taken from P_t = buf[cur] at
// the sampling point: cell for cell what lbm_get_macros returns at steps_done == t + 1.
//   x0 = floor(px), fx = px - x0, x1 = min(x0 + 1, nx - 1); y likewise with ny - 1
//   a = (1 - fx) v(x0, y0) + fx v(x1, y0);  b = (1 - fx) v(x0, y1) + fx v(x1, y1);  v = (1 - fy) a + fy b
// every product and sum rounded to double; a cell whose weight is exactly zero is not read and its term is left out (fx == 0:
// a = v(x0, y0); fy == 0: v = a), so a probe on a node returns that cell's macros bit for bit and reads no neighbour. The probe belongs
// to the strip whose rows hold floor(py); every other strip stores +0.0 for it, so that strips add up like partial force sums.
#pragma once
#include <cmath>
#include "lbm_kernels.hpp"

namespace lbmk {

constexpr int PROBE_THREADS = 256;      // one probe per thread

struct ProbeEntry {
    int x0, y0;         // the cell of floor(px), floor(py); y0 in LOCAL rows of the owning strip (0, 0 where not owned)
    double fx, fy;      // px - x0, py - floor(py), exact (both operands are representable, the difference too)
    int owned, pad;     // floor(py) lies in this strip's rows
};

// The table entry of probe (px, py) for the strip [y_start, y_start + ny_loc) of a lattice nx x ny_glob. The caller has checked that the
// point is finite and inside the domain.
inline ProbeEntry probe_entry(double px, double py, int y_start, int ny_loc) {
    ProbeEntry e;
    const double xf = std::floor(px), yf = std::floor(py);
    const int yg = (int)yf;
    e.owned = (yg >= y_start && yg < y_start + ny_loc) ? 1 : 0;
    e.pad = 0;
    if (e.owned) { e.x0 = (int)xf; e.y0 = yg - y_start; e.fx = px - xf; e.fy = py - yf; }
    else { e.x0 = 0; e.y0 = 0; e.fx = 0.0; e.fy = 0.0; }
    return e;
}

template <typename T>
struct ProbeArgs {
    MacroArgs<T> m;             // the snapshot's source: old = P_t, initial = 0; rho / ux / uy / max_usq_bits unused
    const ProbeEntry* table;    // [n]
    double* out;                // the ring slot: [n][3]
    int n;
};

template <typename T>
void launch_probes(const ProbeArgs<T>& a, hipStream_t s);

}  // namespace lbmk
