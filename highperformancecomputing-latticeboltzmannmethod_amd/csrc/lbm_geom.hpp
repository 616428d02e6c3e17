// csrc/lbm_geom.hpp — host side of a user-defined geometry (lbm_set_solid_mask): the global [ny][nx] byte mask packed into what the
// kernels of ONE strip read (lbm_kernels.hpp MaskView): the bitmap of the rows the strip can ever query — its own rows +- GR, clipped
// to the domain (the fused kernels recompute up to GR ghost rows redundantly) — and the summed-area table of the solid counts of
// 8x8-cell blocks of the same window. Plus what the host needs: the mask's bounding box (force box) and a digest (checkpoints).
#pragma once
#include "lbm_kernels.hpp"

#include <cstdint>
#include <vector>

namespace lbmk {

struct HostMask {
    std::vector<unsigned long long> bits;   // [rows][words]
    std::vector<int> sat;                   // [nby + 1][nbx + 1]
    int y0 = 0, rows = 0, words = 0, nbx = 0, nby = 0;
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;   // bounding box of the solid cells of the WHOLE mask (global, inclusive; empty: x1 < x0)
    unsigned long long digest = 0;              // FNV-1a over nx, ny and the 0/1 cells of the whole mask
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
    unsigned long long d = 1469598103934665603ull;
    auto mix = [&](unsigned v) { d ^= v; d *= 1099511628211ull; };
    mix((unsigned)nx); mix((unsigned)ny);
    h.bx0 = nx; h.by0 = ny;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const bool s = mask[(size_t)y * nx + x] != 0;
            mix(s ? 1u : 0u);
            if (s) {
                h.bx0 = x < h.bx0 ? x : h.bx0; h.bx1 = x > h.bx1 ? x : h.bx1;
                h.by0 = y < h.by0 ? y : h.by0; h.by1 = y > h.by1 ? y : h.by1;
            }
        }
    if (h.bx1 < 0) { h.bx0 = 0; h.by0 = 0; }
    h.digest = d;
    return h;
}

}  // namespace lbmk
