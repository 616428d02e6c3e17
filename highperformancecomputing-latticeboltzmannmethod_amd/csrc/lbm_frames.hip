// csrc/lbm_frames.hip — k_frame: one coarsened flow frame (rho, ux, uy, vorticity; lbm_frames.hpp) from the populations P_t, for both
// element types. A translation unit of its own (build.py): it compiles beside lbm_hip.hip and leaves every step kernel untouched.
//
// A streaming kernel: nine populations read per fine cell, 4 / k^2 floats written. A block of 256 threads owns frame_block_cols(k)
// columns (whole coarse cells; one thread per fine column plus one halo column on either side) and walks frame_band_rows(k) rows
// bottom to top, the nine loads of row y + 1 in flight while row y is finished:
//   dux/dy  from the thread's own three rows of ux, kept in registers (the band starts one row below its first row: at a strip face
//           that row is the ghost row, which holds the neighbour's P_t);
//   duy/dx  from the neighbours' uy of the same row through LDS (two row buffers: one barrier per row);
//   sums    each thread adds its column's k rows; after every k-th row the column sums go to LDS and one thread per coarse value adds
//           k of them, divides by k * k, rounds to float and stores it — consecutive threads store consecutive floats of a plane.
// No tile of macros is staged: a fine cell's macros are needed by four neighbours, and two of them are the thread itself one row
// earlier and later. LDS per block: 12 KB of the CU's 160 KB, so the registers (not LDS) bound the occupancy.
// Interior columns load through buffer descriptors (one per row and population, base in SGPRs, ONE constant 32-bit lane offset for all
// rows and planes: no vector address arithmetic) and form their moments with macro_moments; the inlet and outlet columns — two lanes
// of a row — go through macro_cell itself (pull + wall + Zou-He: on a ghost row that pull reaches the SECOND ghost row of the face).
// Either way the macros are those of k_macros to the bit.
#include "lbm_frames.hpp"

namespace lbmk {

template <typename T>
__global__ void __launch_bounds__(FRAME_THREADS) k_frame(const FrameArgs<T> p) {
#pragma clang fp contract(off)
    __shared__ double s_uy[2][FRAME_THREADS];
    __shared__ double s_col[4][FRAME_THREADS];
    const MacroArgs<T>& a = p.m;
    const int k = p.k;
    const int W = frame_block_cols(k), R = frame_band_rows(k);
    const int tid = (int)threadIdx.x;
    const int X0 = (int)blockIdx.x * W;                     // the block's first fine column
    const int x = X0 - 1 + tid;                             // this thread's column (tid 0 and W + 1: halo)
    const int y0 = (int)blockIdx.y * R;                     // the band's first local row
    const int yend = y0 + R < a.ny_loc ? y0 + R : a.ny_loc;
    const bool have = x >= 0 && x < a.nx && tid <= W + 1;   // a column of the lattice this block reads
    const bool own = have && tid >= 1 && tid <= W;          // ... and sums
    const bool edge = x == 0 || x == a.nx - 1;
    const unsigned voff = have ? (unsigned)((a.xoff + x) * (int)sizeof(T)) : 0u;

    // the nine populations of (x, row y) on their way (interior columns), and the macros they give
    auto load = [&](int y, T (&f)[Q]) {
        if (have && !edge) {
            const T* row = a.old + (long)(y + GR) * a.pitch;
#pragma unroll
            for (int i = 0; i < Q; ++i) f[i] = buf_load<T>(buf_desc(row + (long)i * a.plane), voff, 0u);
        }
    };
    auto finish = [&](int y, const T (&f)[Q], double& r, double& vx, double& vy) {
        r = 0.0; vx = 0.0; vy = 0.0;
        if (!have) return;
        if (edge) { macro_cell<T>(a, x, y, r, vx, vy); return; }
        macro_moments<T>(a, f, r, vx, vy);
        if (solid_at(a, x, a.y_start + y)) { r = 1.0; vx = 0.0; vy = 0.0; }
    };

    T f[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) f[i] = T(0);
    double ux_prev = 0.0, r_cur, ux_cur, uy_cur;
    if (a.y_start + y0 > 0) {      // the row below the band (a ghost row at a strip face): its ux only
        double r_, vy_;
        load(y0 - 1, f);
        finish(y0 - 1, f, r_, ux_prev, vy_);
    }
    load(y0, f);
    finish(y0, f, r_cur, ux_cur, uy_cur);

    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int y = y0; y < yend; ++y) {
        const int yg = a.y_start + y;
        const bool has_next = yg + 1 < a.ny_glob;      // (uniform) the row above exists: in the strip, or the ghost row of its north face
        if (has_next) load(y + 1, f);
        double* uyrow = s_uy[y & 1];
        uyrow[tid] = uy_cur;
        __syncthreads();
        double duy_dx = 0.0;
        if (own) {
            if (x == 0) duy_dx = uyrow[tid + 1] - uy_cur;
            else if (x == a.nx - 1) duy_dx = uy_cur - uyrow[tid - 1];
            else duy_dx = 0.5 * (uyrow[tid + 1] - uyrow[tid - 1]);
        }
        double r_n = 0.0, ux_n = 0.0, uy_n = 0.0;
        if (has_next) finish(y + 1, f, r_n, ux_n, uy_n);
        double dux_dy;
        if (yg == 0) dux_dy = ux_n - ux_cur;
        else if (yg == a.ny_glob - 1) dux_dy = ux_cur - ux_prev;
        else dux_dy = 0.5 * (ux_n - ux_prev);
        if (own) {
            acc[0] = acc[0] + r_cur; acc[1] = acc[1] + ux_cur; acc[2] = acc[2] + uy_cur;
            acc[3] = acc[3] + (duy_dx - dux_dy);
        }
        if ((y - y0 + 1) % k == 0) {      // (uniform) a row of coarse cells is complete
#pragma unroll
            for (int j = 0; j < 4; ++j) { s_col[j][tid] = acc[j]; acc[j] = 0.0; }
            __syncthreads();
            const int wcols = a.nx - X0 < W ? a.nx - X0 : W;
            const int cw = wcols / k;
            const long cells = (long)p.cny * p.cnx;
            const long at = (long)(y / k) * p.cnx + X0 / k;
            const double den = (double)(k * k);
            for (int j = tid; j < 4 * cw; j += FRAME_THREADS) {
                const int pl = j / cw, cc = j - pl * cw;
                const double* q = &s_col[pl][1 + cc * k];
                double s = 0.0;
                for (int i = 0; i < k; ++i) s = s + q[i];
                p.out[(long)pl * cells + at + cc] = (float)(s / den);
            }
            // (the next write to s_col follows the next row's barrier, which every reader above has reached by then)
        }
        ux_prev = ux_cur;
        r_cur = r_n; ux_cur = ux_n; uy_cur = uy_n;
    }
}

template <typename T>
void launch_frame(const FrameArgs<T>& a, hipStream_t s) {
    const int W = frame_block_cols(a.k), R = frame_band_rows(a.k);
    const dim3 grid((a.m.nx + W - 1) / W, (a.m.ny_loc + R - 1) / R), block(FRAME_THREADS);
    hipLaunchKernelGGL((k_frame<T>), grid, block, 0, s, a);
}

template void launch_frame<double>(const FrameArgs<double>&, hipStream_t);
template void launch_frame<float>(const FrameArgs<float>&, hipStream_t);

}  // namespace lbmk
