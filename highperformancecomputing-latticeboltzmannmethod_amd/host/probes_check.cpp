// host/probes_check.cpp — a stand-alone client of host/lbm/probes.hpp (the probe points of lbm_solver --probes / --probe-line), for the
// tests: no device and no GPU library, so it can also be built with -fsanitize=address,undefined.
//   probes_check NX NY [--probes FILE] [--probe-line x0 y0 x1 y1 n] ...
// Prints the points in the order of the options, one `x y` per line at %.17g, after checking them against the NX x NY domain.
// Exit code 2 with the reason on stderr for anything lbm_solver would refuse.
#include "lbm/probes.hpp"

#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: probes_check NX NY [--probes FILE] [--probe-line x0 y0 x1 y1 n] ...\n"); return 2; }
    const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]);
    std::vector<LBM::ProbePoint> pts;
    try {
        for (int a = 3; a < argc; ++a) {
            const std::string k = argv[a];
            std::vector<LBM::ProbePoint> more;
            if (k == "--probes") {
                if (a + 1 >= argc) throw std::runtime_error("missing value for --probes");
                more = LBM::read_probe_file(argv[++a]);
            } else if (k == "--probe-line") {
                if (a + 5 >= argc) throw std::runtime_error("--probe-line takes five values: x0 y0 x1 y1 n");
                more = LBM::parse_probe_line(argv + a + 1);
                a += 5;
            } else throw std::runtime_error("unknown option " + k);
            pts.insert(pts.end(), more.begin(), more.end());
        }
        LBM::check_probe_points(pts, nx, ny);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    for (const LBM::ProbePoint& p : pts) std::printf("%.17g %.17g\n", p.x, p.y);
    return 0;
}
