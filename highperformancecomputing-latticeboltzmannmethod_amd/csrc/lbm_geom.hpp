// csrc/lbm_geom.hpp — host side of a user-defined geometry (lbm_set_solid_mask): the global [ny][nx] byte mask packed into what the
// kernels of ONE strip read (lbm_kernels.hpp MaskView): the bitmap of the rows the strip can ever query — its own rows +- GR, clipped
// to the domain (the fused kernels recompute up to GR ghost rows redundantly) — and the summed-area table of the solid counts of
// 8x8-cell blocks of the same window. Plus what the host needs: the mask's bounding box (force box) and a digest (checkpoints).
#pragma once
#include "lbm_kernels.hpp"
#include "lbm_ckpt.hpp"

#include <cstdint>
#include <cstring>
#include <vector>

namespace lbmk {

struct HostMask {
    std::vector<unsigned long long> bits;   // [rows][words]
    std::vector<int> sat;                   // [nby + 1][nbx + 1]
    int y0 = 0, rows = 0, words = 0, nbx = 0, nby = 0;
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;   // bounding box of the solid cells of the WHOLE mask (global, inclusive; empty: x1 < x0)
    unsigned long long digest = 0;              // of the whole mask (lbm_ckpt.hpp mask_digest)
    MaskView view() const {                     // (host pointers: for the host-side queries and the test hook)
        MaskView m;
        m.bits = bits.data(); m.sat = sat.data();
        m.y0 = y0; m.rows = rows; m.words = words; m.nbx = nbx; m.nby = nby;
        return m;
    }
};

inline HostMask pack_mask(const unsigned char* mask, int nx, int ny, int y_start, int local_ny) {
    HostMask h;
    h.y0 = y_start - GR < 0 ? 0 : y_start - GR;
    const int y1 = y_start + local_ny + GR > ny ? ny : y_start + local_ny + GR;
    h.rows = y1 - h.y0;
    h.words = (nx + 63) / 64;
    h.nbx = (nx + 7) / 8;
    h.nby = (h.rows + 7) / 8;
    h.bits.assign((size_t)h.rows * h.words, 0ull);
    std::vector<int> blocks((size_t)h.nby * h.nbx, 0);
    for (int r = 0; r < h.rows; ++r)
        for (int x = 0; x < nx; ++x)
            if (mask[(size_t)(h.y0 + r) * nx + x]) {
                h.bits[(size_t)r * h.words + (x >> 6)] |= 1ull << (x & 63);
                blocks[(size_t)(r >> 3) * h.nbx + (x >> 3)] += 1;
            }
    const int W = h.nbx + 1;
    h.sat.assign((size_t)(h.nby + 1) * W, 0);
    for (int b = 0; b < h.nby; ++b)
        for (int c = 0; c < h.nbx; ++c)
            h.sat[(size_t)(b + 1) * W + c + 1] = blocks[(size_t)b * h.nbx + c] + h.sat[(size_t)b * W + c + 1] +
                                                 h.sat[(size_t)(b + 1) * W + c] - h.sat[(size_t)b * W + c];
    h.bx0 = nx; h.by0 = ny;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x)
            if (mask[(size_t)y * nx + x]) {
                h.bx0 = x < h.bx0 ? x : h.bx0; h.bx1 = x > h.bx1 ? x : h.bx1;
                h.by0 = y < h.by0 ? y : h.by0; h.by1 = y > h.by1 ? y : h.by1;
            }
    if (h.bx1 < 0) { h.bx0 = 0; h.by0 = 0; }
    h.digest = mask_digest(mask, nx, ny);
    return h;
}

// Periodic y (lbm_set_periodic_y): the window of a strip whose kernels count rows from `pad` rows below the lattice (lbm_launch.inc.hpp
// row_offset): rows y_start + pad - GR .. y_start + pad + local_ny + GR - 1 in that count, ALL of them (no clipping: every one is a
// row of the repeated lattice), row r of the count being S(x, (r - pad) mod ny). `solid(x, w, y)` answers for window row w, which is
// lattice row y: the user's mask (kept by window row, wrapped_rows below) or the disc test. The bounding box is that of the WINDOW, in
// the same count (the force box: the images across the seam belong to it); no digest (a checkpoint describes what the user set).
template <typename Solid>
inline HostMask pack_mask_periodic(Solid&& solid, int nx, int ny, int y_start, int local_ny, int pad) {
    HostMask h;
    h.y0 = y_start + pad - GR;
    h.rows = local_ny + 2 * GR;
    h.words = (nx + 63) / 64;
    h.nbx = (nx + 7) / 8;
    h.nby = (h.rows + 7) / 8;
    h.bits.assign((size_t)h.rows * h.words, 0ull);
    std::vector<int> blocks((size_t)h.nby * h.nbx, 0);
    h.bx0 = nx; h.by0 = h.y0 + h.rows;
    for (int r = 0; r < h.rows; ++r) {
        const int y = ((h.y0 + r - pad) % ny + ny) % ny;
        for (int x = 0; x < nx; ++x)
            if (solid(x, r, y)) {
                h.bits[(size_t)r * h.words + (x >> 6)] |= 1ull << (x & 63);
                blocks[(size_t)(r >> 3) * h.nbx + (x >> 3)] += 1;
                h.bx0 = x < h.bx0 ? x : h.bx0; h.bx1 = x > h.bx1 ? x : h.bx1;
                h.by0 = h.y0 + r < h.by0 ? h.y0 + r : h.by0; h.by1 = h.y0 + r > h.by1 ? h.y0 + r : h.by1;
            }
    }
    const int W = h.nbx + 1;
    h.sat.assign((size_t)(h.nby + 1) * W, 0);
    for (int b = 0; b < h.nby; ++b)
        for (int c = 0; c < h.nbx; ++c)
            h.sat[(size_t)(b + 1) * W + c + 1] = blocks[(size_t)b * h.nbx + c] + h.sat[(size_t)b * W + c + 1] +
                                                 h.sat[(size_t)(b + 1) * W + c] - h.sat[(size_t)b * W + c];
    if (h.bx1 < 0) { h.bx0 = 0; h.by0 = 0; }
    return h;
}

// ... and the rows of a global [ny][nx] mask that window holds, [local_ny + 2 GR][nx], wrapped: what a context keeps of the user's mask
// in case it is made periodic (the setters may come in either order)
inline std::vector<unsigned char> wrapped_rows(const unsigned char* mask, int nx, int ny, int y_start, int local_ny) {
    std::vector<unsigned char> w((size_t)(local_ny + 2 * GR) * nx);
    for (int r = 0; r < local_ny + 2 * GR; ++r) memcpy(&w[(size_t)r * nx], mask + (size_t)(((y_start - GR + r) % ny + ny) % ny) * nx, (size_t)nx);
    return w;
}

// Per-body force reporting (lbm_set_body_labels): what k_forces_bodies reads for ONE strip of a global [ny][nx] label array
// (0 fluid, k = 1..255 a solid cell of body k; B = the largest label present, a label nobody carries is a body without cells).
//   lab    [(local_ny + 2)][nx]: the strip's rows and one ghost row per face, zeros beyond the domain
//   box    [B][4]: body k's bounding box + 1 cell, clipped to the domain and to the strip's rows, x0, x1, y0, y1 inclusive in
//          (x, LOCAL y) — the rule of k_forces' one box, per body; {0, -1, 0, -1} where nothing of it lies in the strip
//   chunks every non-empty box in row-major runs of FORCE_CHUNK cells, bodies in label order: the blocks of one sample
//   first  [B + 1]: body k's chunks are [first[k - 1], first[k])
struct HostBodies {
    int B = 0;
    std::vector<unsigned char> lab;
    std::vector<int> box;
    std::vector<BodyChunk> chunks;
    std::vector<int> first;
};

inline HostBodies pack_bodies(const unsigned char* labels, int nx, int ny, int y_start, int local_ny) {
    HostBodies h;
    int bx0[256], bx1[256], by0[256], by1[256];
    long cells[256];
    for (int k = 0; k < 256; ++k) { bx0[k] = nx; bx1[k] = -1; by0[k] = ny; by1[k] = -1; cells[k] = 0; }
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const int k = labels[(size_t)y * nx + x];
            if (!k) continue;
            h.B = k > h.B ? k : h.B;
            cells[k]++;
            bx0[k] = x < bx0[k] ? x : bx0[k]; bx1[k] = x > bx1[k] ? x : bx1[k];
            by0[k] = y < by0[k] ? y : by0[k]; by1[k] = y > by1[k] ? y : by1[k];
        }
    h.lab.assign((size_t)(local_ny + 2) * nx, 0);
    for (int r = 0; r < local_ny + 2; ++r) {
        const int y = y_start - 1 + r;
        if (y >= 0 && y < ny) memcpy(&h.lab[(size_t)r * nx], labels + (size_t)y * nx, (size_t)nx);
    }
    h.first.assign(1, 0);
    for (int k = 1; k <= h.B; ++k) {
        int b[4] = {0, -1, 0, -1};
        if (cells[k] > 0) {
            const int x0 = bx0[k] - 1 < 0 ? 0 : bx0[k] - 1, x1 = bx1[k] + 1 > nx - 1 ? nx - 1 : bx1[k] + 1;
            const int y0 = by0[k] - 1 - y_start < 0 ? 0 : by0[k] - 1 - y_start;
            const int y1 = by1[k] + 1 - y_start > local_ny - 1 ? local_ny - 1 : by1[k] + 1 - y_start;
            if (y1 >= y0) { b[0] = x0; b[1] = x1; b[2] = y0; b[3] = y1; }
        }
        h.box.insert(h.box.end(), b, b + 4);
        const long ncell = b[1] >= b[0] ? (long)(b[1] - b[0] + 1) * (b[3] - b[2] + 1) : 0;
        for (long f = 0; f < ncell; f += FORCE_CHUNK) {
            BodyChunk c;
            c.body = k; c.first = f; c.cells = (int)(ncell - f < FORCE_CHUNK ? ncell - f : FORCE_CHUNK);
            h.chunks.push_back(c);
        }
        h.first.push_back((int)h.chunks.size());
    }
    return h;
}

}  // namespace lbmk
