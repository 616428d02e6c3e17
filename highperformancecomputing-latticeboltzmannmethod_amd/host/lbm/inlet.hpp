// host/lbm/inlet.hpp — inlet velocity profiles for lbm_solver --inlet-profile parabolic|FILE: a SHAPE over the ny rows (the
// Poiseuille parabola s(1-s), s = (y + 0.5)/ny, or ny numbers read from a text file, row 0 = bottom first), scaled so that its mean
// over the rows equals inlet_velocity. The mean velocity therefore stays the run's reference velocity (Reynolds number, Cd / Cl).
// Built and checked on the host before any device is touched; the result is the array of absolute velocities that
// lbm_set_inlet_profile takes. The Python helper parabolic_profile (binding.py) restates parabolic_inlet_shape and
// scale_inlet_profile operation by operation.
#pragma once
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace LBM {

inline std::vector<double> parabolic_inlet_shape(int ny) {
    std::vector<double> s((size_t)ny);
    for (int y = 0; y < ny; ++y) {
        const double t = (y + 0.5) / ny;
        s[(size_t)y] = t * (1.0 - t);
    }
    return s;
}

// u[y] = shape[y] * (mean / (sum of the shape, rows in order, / ny)). Throws when the shape's mean is not positive or a scaled value
// is not below 1 (the Zou-He inlet divides by 1 - u).
inline std::vector<double> scale_inlet_profile(const std::vector<double>& shape, double mean, const std::string& what) {
    double sum = 0.0;
    for (double v : shape) sum += v;
    const double shape_mean = sum / (double)shape.size();
    if (!(shape_mean > 0.0) || !std::isfinite(shape_mean))
        throw std::runtime_error("inlet profile " + what + ": the mean of the shape must be positive");
    const double scale = mean / shape_mean;
    std::vector<double> u(shape.size());
    for (size_t y = 0; y < shape.size(); ++y) {
        u[y] = shape[y] * scale;
        if (!(u[y] < 1.0) || !std::isfinite(u[y]))
            throw std::runtime_error("inlet profile " + what + ": row " + std::to_string(y) + " scales to " + std::to_string(u[y]) +
                                     " (velocities must stay below 1)");
    }
    return u;
}

// The shape in a text file: ny numbers, row 0 (bottom) first, separated by white space; '#' starts a comment to the end of the line.
// Throws with the reason: unreadable file, a token that is not a number, a value that is not finite, a count other than ny.
inline std::vector<double> read_inlet_shape(const std::string& path, int ny) {
    std::FILE* fp = std::fopen(path.c_str(), "r");
    if (!fp) throw std::runtime_error("cannot open inlet profile " + path);
    struct Closer { std::FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
    auto bad = [&](const std::string& why) { return std::runtime_error("inlet profile " + path + ": " + why); };
    std::vector<double> s;
    std::string tok;
    int line = 1;
    auto take = [&]() {
        if (tok.empty()) return;
        char* end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end != '\0') throw bad("line " + std::to_string(line) + ": '" + tok + "' is not a number");
        if (!std::isfinite(v)) throw bad("line " + std::to_string(line) + ": '" + tok + "' is not finite");
        s.push_back(v);
        tok.clear();
    };
    for (int ch = std::fgetc(fp); ch != EOF; ch = std::fgetc(fp)) {
        if (ch == '#') {
            take();
            while (ch != EOF && ch != '\n') ch = std::fgetc(fp);
            if (ch == EOF) break;
        }
        if (std::isspace(ch)) {
            take();
            if (ch == '\n') ++line;
        } else {
            tok.push_back((char)ch);
        }
    }
    take();
    if ((long)s.size() != ny) throw bad(std::to_string(s.size()) + " values, the lattice has ny = " + std::to_string(ny) + " rows");
    return s;
}

// --inlet-profile SPEC: "parabolic" or a file of the shape, scaled to the mean velocity `mean`.
inline std::vector<double> build_inlet_profile(const std::string& spec, int ny, double mean) {
    if (ny < 1) throw std::runtime_error("inlet profile: ny must be positive");
    if (spec == "parabolic") return scale_inlet_profile(parabolic_inlet_shape(ny), mean, spec);
    return scale_inlet_profile(read_inlet_shape(spec, ny), mean, spec);
}

}  // namespace LBM
