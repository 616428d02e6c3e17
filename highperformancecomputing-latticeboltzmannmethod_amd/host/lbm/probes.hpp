// host/lbm/probes.hpp — the probe points of lbm_solver --probes FILE / --probe-line x0 y0 x1 y1 n: points (x, y) in global lattice
// coordinates at which the device samples (rho, ux, uy) by bilinear interpolation at every output iteration (lbm_probes_begin; the
// reference has none). Parsed, expanded and checked on the host before any device is touched; the result is the [n][2] array that
// lbm_probes_begin takes. Depends on the standard library alone (host/probes_check.cpp runs it without the GPU library).
#pragma once
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace LBM {

struct ProbePoint { double x, y; };

inline constexpr int PROBES_MAX = 65536;   // LBM_PROBES_MAX

// One number of a probe option or file; throws with `what` and the token when it is not a finite number.
inline double probe_number(const std::string& tok, const std::string& what) {
    char* end = nullptr;
    const double v = std::strtod(tok.c_str(), &end);
    if (tok.empty() || end == tok.c_str() || *end != '\0') throw std::runtime_error(what + ": '" + tok + "' is not a number");
    if (!std::isfinite(v)) throw std::runtime_error(what + ": '" + tok + "' is not finite");
    return v;
}

// n equally spaced points from (x0, y0) to (x1, y1), end points included: point j = p0 + (p1 - p0) * j / (n - 1) (the product first),
// the last one (x1, y1) itself; n == 1 gives (x0, y0). Every point lies in the box the end points span.
inline std::vector<ProbePoint> expand_probe_line(double x0, double y0, double x1, double y1, int n) {
    if (n < 1 || n > PROBES_MAX) throw std::runtime_error("--probe-line: n = " + std::to_string(n) + " outside 1.." + std::to_string(PROBES_MAX));
    auto at = [n](double a, double b, int j) {
        if (j == 0) return a;
        if (j == n - 1) return b;
        const double v = a + (b - a) * (double)j / (double)(n - 1);
        const double lo = a < b ? a : b, hi = a < b ? b : a;
        return v < lo ? lo : v > hi ? hi : v;
    };
    std::vector<ProbePoint> pts((size_t)n);
    for (int j = 0; j < n; ++j) pts[(size_t)j] = {at(x0, x1, j), at(y0, y1, j)};
    return pts;
}

// The five values of one --probe-line option, as the command line gives them.
inline std::vector<ProbePoint> parse_probe_line(const char* const* args5) {
    double v[4];
    for (int k = 0; k < 4; ++k) v[k] = probe_number(args5[k], "--probe-line");
    char* end = nullptr;
    const long n = std::strtol(args5[4], &end, 10);
    if (end == args5[4] || *end != '\0' || n < 1 || n > PROBES_MAX)
        throw std::runtime_error(std::string("--probe-line: '") + args5[4] + "' is not a number of points in 1.." + std::to_string(PROBES_MAX));
    return expand_probe_line(v[0], v[1], v[2], v[3], (int)n);
}

// --probes FILE: one `x y` per line, separated by white space; '#' starts a comment to the end of the line; blank lines are skipped.
// Throws with the reason: unreadable file, a token that is not a finite number, a line with other than two numbers, no point at all.
inline std::vector<ProbePoint> read_probe_file(const std::string& path) {
    std::FILE* fp = std::fopen(path.c_str(), "r");
    if (!fp) throw std::runtime_error("cannot open probe file " + path);
    struct Closer { std::FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
    std::vector<ProbePoint> pts;
    std::vector<double> vals;      // the numbers of the current line
    std::string tok;
    int line = 1;
    auto where = [&]() { return "probe file " + path + ": line " + std::to_string(line); };
    auto take = [&]() {
        if (tok.empty()) return;
        vals.push_back(probe_number(tok, where()));
        tok.clear();
    };
    auto end_line = [&]() {
        take();
        if (vals.size() == 2) pts.push_back({vals[0], vals[1]});
        else if (!vals.empty()) throw std::runtime_error(where() + ": " + std::to_string(vals.size()) + " numbers, a probe is `x y`");
        vals.clear();
        ++line;
    };
    bool comment = false;
    for (int ch = std::fgetc(fp); ch != EOF; ch = std::fgetc(fp)) {
        if (ch == '\n') { end_line(); comment = false; }
        else if (comment) continue;
        else if (ch == '#') { take(); comment = true; }
        else if (std::isspace(ch)) take();
        else tok.push_back((char)ch);
    }
    end_line();
    if (pts.empty()) throw std::runtime_error("probe file " + path + ": no probe point");
    return pts;
}

// What lbm_probes_begin would refuse, found before a device opens: no more than PROBES_MAX points, each inside 0..nx-1 x 0..ny-1.
inline void check_probe_points(const std::vector<ProbePoint>& pts, int nx, int ny) {
    if ((long)pts.size() > PROBES_MAX) throw std::runtime_error("probes: " + std::to_string(pts.size()) + " points, at most " + std::to_string(PROBES_MAX));
    for (size_t j = 0; j < pts.size(); ++j) {
        const ProbePoint& p = pts[j];
        if (!std::isfinite(p.x) || !std::isfinite(p.y) || p.x < 0.0 || p.x > (double)(nx - 1) || p.y < 0.0 || p.y > (double)(ny - 1)) {
            char b[192];
            std::snprintf(b, sizeof(b), "probe %zu: (%.17g, %.17g) outside the domain 0..%d x 0..%d", j, p.x, p.y, nx - 1, ny - 1);
            throw std::runtime_error(b);
        }
    }
}

}  // namespace LBM
