// csrc/lbm_frames.hpp — what the host translation unit (lbm_hip.hip) sees of the frame kernel (lbm_frames_begin; the reference has
// none): its block geometry, its arguments and one launcher per element type. The kernel itself is compiled in its own translation
// unit (lbm_frames.hip), beside the others (build.py).
//
// The FRAME of iteration t with stride k: four planes [ny_loc / k][nx / k] of float — rho, ux, uy, vorticity — each value the mean over
// its k x k fine cells of
//   (rho, ux, uy)  the snapshot macro_cell defines (lbm_kernels.hpp), taken from P_t = buf[cur] at the sampling point: cell for cell
//                  what lbm_get_macros returns at steps_done == t + 1;
//   w              duy/dx - dux/dy of that snapshot in double: 0.5 * (v[+1] - v[-1]) inside, v[1] - v[0] and v[n-1] - v[n-2] on the
//                  four edges of the DOMAIN (global columns 0, nx - 1 and rows 0, ny - 1: a strip face is interior and takes its
//                  neighbour from the ghost row); solid cells enter with the (0, 0) the snapshot gives them and get their w alike.
// Summation order of a coarse value: per fine column the k rows bottom to top, then the k column sums left to right; then one division
// by k * k and one rounding to float. The order depends on k alone, so every plan, layout, arithmetic mode of the step kernels and
// strip decomposition gives the same bits for the same macros.
#pragma once
#include "lbm_kernels.hpp"

namespace lbmk {

constexpr int FRAME_THREADS = 256;      // one fine column per thread: the block's columns and one halo column on either side
constexpr int FRAME_MAX_K = 64;
constexpr int FRAME_BAND = 16;          // fine rows a block walks (k > 16: k): 1 / 8 more rows read than stored, four blocks per CU at 4096x1024
constexpr int frame_block_cols(int k) { return ((FRAME_THREADS - 2) / k) * k; }        // whole coarse cells: 254 (k = 1) ... 192 (k = 64)
constexpr int frame_band_rows(int k) { return k >= FRAME_BAND ? k : (FRAME_BAND / k) * k; }

template <typename T>
struct FrameArgs {
    MacroArgs<T> m;     // the snapshot's source: old = P_t, initial = 0; rho / ux / uy / max_usq_bits unused
    float* out;         // the ring slot: [4][cny][cnx]
    int k, cnx, cny;    // stride; nx / k, ny_loc / k
};

template <typename T>
void launch_frame(const FrameArgs<T>& a, hipStream_t s);

}  // namespace lbmk
