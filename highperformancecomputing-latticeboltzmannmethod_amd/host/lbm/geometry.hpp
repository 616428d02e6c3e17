// host/lbm/geometry.hpp — obstacle masks for lbm_solver --obstacle-mask: a binary (P5) or ASCII (P2) PGM of exactly nx x ny
// pixels, a pixel is solid when it is nonzero. The file's FIRST image row is lattice row ny-1, so the picture looks like the VTK
// view (y up). Parsed and checked on the host before any device is touched; the result is the global [ny][nx] byte mask that
// lbm_set_solid_mask takes (row y = 0 first).
// lbm_solver --obstacle-bodies reads the same file format with the grey value kept as the body number (0 fluid, k = 1..255 a cell of
// body k): the array lbm_set_body_labels takes, plus each body's cell count and frontal height.
#pragma once
#include <cctype>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace LBM {

struct ObstacleMask {
    std::vector<unsigned char> cells;   // [ny][nx], row 0 = bottom; 1 = solid
    int frontal_height = 0;             // rows that hold a solid cell: the reference length D of a masked run
    int solid_cells = 0;
    // read_obstacle_pgm(..., keep_labels): cells hold the grey values; per body k = 1..B (index k - 1) its cells and the rows it spans
    // (last row - first row + 1: the reference length D of that body's coefficients; 0 for a label nobody carries)
    std::vector<int> body_cells, body_height;
};

namespace detail {
// next header token of a PGM: skips whitespace and '#' comments (to the end of the line)
inline bool pgm_token(std::FILE* fp, std::string& tok) {
    tok.clear();
    int ch = std::fgetc(fp);
    for (;;) {
        while (ch != EOF && std::isspace(ch)) ch = std::fgetc(fp);
        if (ch != '#') break;
        while (ch != EOF && ch != '\n') ch = std::fgetc(fp);
    }
    while (ch != EOF && !std::isspace(ch) && ch != '#') { tok.push_back((char)ch); ch = std::fgetc(fp); }
    if (ch == '#') std::ungetc(ch, fp);
    return !tok.empty();   // (a P5 header ends on the single whitespace character consumed here)
}
inline bool pgm_int(std::FILE* fp, long& v) {
    std::string t;
    if (!pgm_token(fp, t) || t.size() > 9) return false;
    for (char c : t) if (!std::isdigit((unsigned char)c)) return false;
    v = std::stol(t);
    return true;
}
}  // namespace detail

// Throws std::runtime_error with the reason: unreadable file, bad header, wrong size, maxval outside 1..255, short or bad data.
// what: how the messages name the file ("obstacle mask" / "--obstacle-bodies"); keep_labels: see ObstacleMask.
inline ObstacleMask read_obstacle_pgm(const std::string& path, int nx, int ny, const std::string& what = "obstacle mask", bool keep_labels = false) {
    std::FILE* fp = std::fopen(path.c_str(), "rb");
    if (!fp) throw std::runtime_error("cannot open " + what + " " + path);
    struct Closer { std::FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
    auto bad = [&](const std::string& why) { return std::runtime_error(what + " " + path + ": " + why); };
    std::string magic;
    if (!detail::pgm_token(fp, magic) || (magic != "P5" && magic != "P2")) throw bad("not a PGM file (magic P5 or P2 expected)");
    long w = 0, h = 0, maxval = 0;
    if (!detail::pgm_int(fp, w) || !detail::pgm_int(fp, h) || !detail::pgm_int(fp, maxval)) throw bad("bad PGM header");
    if (w != nx || h != ny)
        throw bad("image is " + std::to_string(w) + "x" + std::to_string(h) + ", the lattice " + std::to_string(nx) + "x" + std::to_string(ny));
    if (maxval < 1 || maxval > 255) throw bad("maxval " + std::to_string(maxval) + " (1..255 supported)");
    ObstacleMask m;
    m.cells.assign((size_t)nx * ny, 0);
    std::vector<unsigned char> row((size_t)nx);
    for (int r = 0; r < ny; ++r) {   // image row r = lattice row ny-1-r
        if (magic == "P5") {
            if (std::fread(row.data(), 1, row.size(), fp) != row.size()) throw bad("short pixel data");
        } else {
            for (int x = 0; x < nx; ++x) {
                long v = 0;
                if (!detail::pgm_int(fp, v)) throw bad("short or bad pixel data");
                if (v > maxval) throw bad("pixel value above maxval");
                row[(size_t)x] = (unsigned char)v;
            }
        }
        bool any = false;
        unsigned char* dst = m.cells.data() + (size_t)(ny - 1 - r) * nx;
        for (int x = 0; x < nx; ++x) {
            dst[x] = keep_labels ? row[(size_t)x] : (row[(size_t)x] ? 1 : 0);
            any |= dst[x] != 0;
            m.solid_cells += dst[x] != 0;
        }
        m.frontal_height += any ? 1 : 0;
    }
    if (m.solid_cells == 0) throw bad("no solid pixel (the reference length of the force coefficients would be zero)");
    if (keep_labels) {
        std::vector<int> lo(256, ny), hi(256, -1), cells(256, 0);
        int B = 0;
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const int k = m.cells[(size_t)y * nx + x];
                if (!k) continue;
                B = k > B ? k : B;
                cells[(size_t)k]++;
                lo[(size_t)k] = y < lo[(size_t)k] ? y : lo[(size_t)k];
                hi[(size_t)k] = y > hi[(size_t)k] ? y : hi[(size_t)k];
            }
        for (int k = 1; k <= B; ++k) {
            m.body_cells.push_back(cells[(size_t)k]);
            m.body_height.push_back(cells[(size_t)k] ? hi[(size_t)k] - lo[(size_t)k] + 1 : 0);
        }
    }
    return m;
}

}  // namespace LBM
