// csrc/lbm_gather.hpp — how the results of the row strips of one lattice are put together: the index arithmetic and the one order of
// summation behind every lbm_group_* gather (lbm_group.inc.hpp). Pure host C++ on host pointers (no HIP, no device), like lbm_plan.hpp:
// the library exports it through lbm_debug_gather so that the rules can be held against numpy on the CPU
// (tests/test_group_gather_cpu.py). What it replaces in the reference: the MPI_Gatherv displacements of Solver::write_vtk_frame
// (LBMSolver.h:340-357) and the MPI_Reduce(SUM) of IOManager::record_forces (LBMIO.h:167-168).
#pragma once
#include <algorithm>
#include <cstddef>

namespace lbmk {

// The rows [y0, y0 + rows) a strip owns of a lattice of ny rows of nx cells, in cells of whatever grid the planes are sampled on.
struct StripRows { size_t nx, ny, y0, rows; };
// ... on the grid of k x k blocks (frames; k divides all four: lbm_frames_begin): a frame is stacked at row y_start / k
inline StripRows coarsen(const StripRows& s, int k) { return {s.nx / (size_t)k, s.ny / (size_t)k, s.y0 / (size_t)k, s.rows / (size_t)k}; }
// where a strip's first row lies in a plane of the whole lattice (lbm_group_get_macros hands this address to the member: no staging copy)
inline size_t plane_offset(const StripRows& s) { return s.y0 * s.nx; }

// P planes of a strip, part = [P][rows][nx], into their place in whole = [P][ny][nx]
template <typename E>
void stack_planes(E* whole, const E* part, int P, const StripRows& s) {
    const size_t m = s.rows * s.nx;
    for (int j = 0; j < P; ++j) std::copy(part + (size_t)j * m, part + ((size_t)j + 1) * m, whole + (size_t)j * s.ny * s.nx + plane_offset(s));
}
// the inverse: the strip's P planes cut out of the whole (lbm_group_stats_restore)
template <typename E>
void unstack_planes(E* part, const E* whole, int P, const StripRows& s) {
    const size_t m = s.rows * s.nx;
    for (int j = 0; j < P; ++j) {
        const E* src = whole + (size_t)j * s.ny * s.nx + plane_offset(s);
        std::copy(src, src + m, part + (size_t)j * m);
    }
}

// Ghost-inclusive populations, part = [rows + 2][row] into whole = [ny + 2][row] (row = (nx + 2) * 9 doubles): every strip gives its
// interior rows; the ghost row of a face is physical — and given — only on the first strip (south) and on the last (north).
inline void stack_populations(double* whole, const double* part, size_t row, const StripRows& s, bool first_strip, bool last_strip) {
    const size_t lo = first_strip ? 0 : 1, hi = s.rows + (last_strip ? 2 : 1);
    std::copy(part + lo * row, part + hi * row, whole + (s.y0 + lo) * row);
}

// The one order of every sum over the strips: strip 0's value, then += strips 1 .. n-1 in that order (no leading 0 +: a lone -0.0 stays).
inline void accumulate(double* total, const double* part, size_t n, bool first_strip) {
    if (first_strip) std::copy(part, part + n, total);
    else for (size_t q = 0; q < n; ++q) total[q] += part[q];
}

}  // namespace lbmk
