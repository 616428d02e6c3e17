// host/lbm/inlet.hpp — inlet velocity profiles for lbm_solver --inlet-profile parabolic|FILE: a SHAPE over the ny rows (the
// Poiseuille parabola s(1-s), s = (y + 0.5)/ny, or ny numbers read from a text file, row 0 = bottom first), scaled so that its mean
// over the rows equals inlet_velocity. The mean velocity therefore stays the run's reference velocity (Reynolds number, Cd / Cl).
// Built and checked on the host before any device is touched; the result is the array of absolute velocities that
// lbm_set_inlet_profile takes. The Python helper parabolic_profile (binding.py) restates parabolic_inlet_shape and
// scale_inlet_profile operation by operation.
// Inlet schedules for lbm_solver --inlet-ramp N | --inlet-pulse A:P | --inlet-schedule FILE: one scale factor of the inflow per
// iteration (lbm_set_inlet_schedule), likewise built and checked before any device is touched; the Python helpers cosine_ramp and
// sine_pulse restate the two builders operation by operation.
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

// The numbers of a text file, separated by white space; '#' starts a comment to the end of the line. `what` names the file's role in
// the messages ("inlet profile", "inlet schedule"). Throws with the reason: unreadable file, a token that is not a number, a value that
// is not finite.
inline std::vector<double> read_inlet_numbers(const std::string& path, const std::string& what) {
    std::FILE* fp = std::fopen(path.c_str(), "r");
    if (!fp) throw std::runtime_error("cannot open " + what + " " + path);
    struct Closer { std::FILE* f; ~Closer() { std::fclose(f); } } closer{fp};
    auto bad = [&](const std::string& why) { return std::runtime_error(what + " " + path + ": " + why); };
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
    return s;
}

// The shape in a text file: ny numbers, row 0 (bottom) first. Throws like read_inlet_numbers, and for a count other than ny.
inline std::vector<double> read_inlet_shape(const std::string& path, int ny) {
    std::vector<double> s = read_inlet_numbers(path, "inlet profile");
    if ((long)s.size() != ny)
        throw std::runtime_error("inlet profile " + path + ": " + std::to_string(s.size()) + " values, the lattice has ny = " + std::to_string(ny) + " rows");
    return s;
}

// --inlet-profile SPEC: "parabolic" or a file of the shape, scaled to the mean velocity `mean`.
inline std::vector<double> build_inlet_profile(const std::string& spec, int ny, double mean) {
    if (ny < 1) throw std::runtime_error("inlet profile: ny must be positive");
    if (spec == "parabolic") return scale_inlet_profile(parabolic_inlet_shape(ny), mean, spec);
    return scale_inlet_profile(read_inlet_shape(spec, ny), mean, spec);
}

// ---- schedules: one scale factor of the inflow per iteration ----
constexpr int INLET_SCHEDULE_MAX = 1048576;   // LBM_INLET_SCHEDULE_MAX

// --inlet-ramp N: N + 1 factors 0.5 * (1 - cos(pi * k / N)), from 0 (rest) to 1; the last one holds.
inline std::vector<double> cosine_ramp(int n) {
    const double pi = 3.141592653589793;
    std::vector<double> s((size_t)n + 1);
    for (int k = 0; k <= n; ++k) s[(size_t)k] = 0.5 * (1.0 - std::cos(pi * (double)k / (double)n));
    return s;
}
// --inlet-pulse A:P: P factors 1 + A * sin(2 * pi * k / P), repeated.
inline std::vector<double> sine_pulse(double amplitude, int period) {
    const double pi = 3.141592653589793;
    std::vector<double> s((size_t)period);
    for (int k = 0; k < period; ++k) s[(size_t)k] = 1.0 + amplitude * std::sin(2.0 * pi * (double)k / (double)period);
    return s;
}
// a whole decimal number in [lo, hi] (std::invalid_argument naming the option otherwise)
inline int parse_schedule_int(const std::string& option, const std::string& text, long lo, long hi) {
    char* end = nullptr;
    const long v = std::strtol(text.c_str(), &end, 10);
    if (text.empty() || end == text.c_str() || *end != '\0' || v < lo || v > hi)
        throw std::invalid_argument(option + ": '" + text + "' is not a whole number in " + std::to_string(lo) + ".." + std::to_string(hi));
    return (int)v;
}
// N of --inlet-ramp -> the table
inline std::vector<double> parse_inlet_ramp(const std::string& text) {
    return cosine_ramp(parse_schedule_int("--inlet-ramp", text, 1, INLET_SCHEDULE_MAX - 1));
}
// A:P of --inlet-pulse -> the table
inline std::vector<double> parse_inlet_pulse(const std::string& text) {
    const size_t colon = text.find(':');
    if (colon == std::string::npos) throw std::invalid_argument("--inlet-pulse: '" + text + "' is not AMPLITUDE:PERIOD");
    const std::string a = text.substr(0, colon);
    char* end = nullptr;
    const double amp = std::strtod(a.c_str(), &end);
    if (a.empty() || end == a.c_str() || *end != '\0' || !std::isfinite(amp))
        throw std::invalid_argument("--inlet-pulse: '" + a + "' is not a finite amplitude");
    return sine_pulse(amp, parse_schedule_int("--inlet-pulse", text.substr(colon + 1), 1, INLET_SCHEDULE_MAX));
}
// FILE of --inlet-schedule -> the table: 1 .. INLET_SCHEDULE_MAX finite numbers
inline std::vector<double> read_inlet_schedule(const std::string& path) {
    std::vector<double> s = read_inlet_numbers(path, "inlet schedule");
    if (s.empty() || (long)s.size() > INLET_SCHEDULE_MAX)
        throw std::runtime_error("inlet schedule " + path + ": " + std::to_string(s.size()) + " values (1 .. " + std::to_string(INLET_SCHEDULE_MAX) + " only)");
    return s;
}
// The inlet divides by 1 - u[y] * s[k]: throws naming row and entry unless every product is below 1. `u`: the profile, or one value
// for the plug inflow.
inline void check_inlet_schedule(const std::vector<double>& u, const std::vector<double>& s) {
    double smin = s[0], smax = s[0];
    for (double v : s) { smin = v < smin ? v : smin; smax = v > smax ? v : smax; }
    for (size_t y = 0; y < u.size(); ++y)
        for (size_t k = 0; k < s.size() && !(u[y] * smin < 1.0 && u[y] * smax < 1.0); ++k)
            if (!(u[y] * s[k] < 1.0))
                throw std::runtime_error("inlet schedule: inlet row " + std::to_string(y) + " (velocity " + std::to_string(u[y]) + ") times entry " +
                                         std::to_string(k) + " (factor " + std::to_string(s[k]) + ") is not below 1");
}

}  // namespace LBM
