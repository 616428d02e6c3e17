// host/main.cpp — lbm_solver: the reference's driver sequence (src/main.cpp:11-20: params -> Solver -> IOManager ->
// initialise -> run -> write_final_results) on the MI355X backend, plus what the reference lacks: command-line
// overrides for every SimulationParams field and backend options.
#include "compat/LBMConfig.h"
#include "compat/LBMIO.h"
#include "compat/LBMSolver.h"
#include "lbm/geometry.hpp"
#include "lbm/inlet.hpp"
#include "lbm/probes.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

static void usage() {
    std::puts("lbm_solver [--nx N] [--ny N] [--steps N] [--output-frequency N] [--tau X] [--inlet-velocity X]\n"
              "           [--reynolds RE] [--cylinder-x F] [--cylinder-y F] [--cylinder-radius F] [--vtk-start-step N]\n"
              "           [--no-vtk] [--no-final] [--sync-vtk] [--fp32] [--contracted] [--no-tune] [--device D] [--quiet]\n"
              "           [--gpus N] [--strips N] [--rccl]\n"
              "           [--checkpoint FILE] [--restart FILE] [--obstacle-mask FILE.pgm] [--obstacle-bodies FILE.pgm]\n"
              "           [--inlet-profile parabolic|FILE] [--print-inlet-profile] [--smagorinsky CS] [--trt-magic LAMBDA]\n"
              "           [--forcing FX,FY] [--mrt BULK,MAGIC] [--sponge WIDTH:TAU_END]\n"
              "           [--stats-start N] [--wall-south KIND] [--wall-north KIND] [--walls KIND]\n"
              "           [--inlet velocity|pressure:RHO] [--outlet pressure:RHO|velocity:U]\n"
              "           [--frame-stride K] [--probes FILE] [--probe-line x0 y0 x1 y1 n]\n"
              "           [--inlet-ramp N | --inlet-pulse A:P | --inlet-schedule FILE [--inlet-schedule-repeat]] [--print-inlet-schedule]\n"
              "Defaults are the reference's SimulationParams (LBMConfig.h:37-51). --reynolds sets the inlet velocity\n"
              "from tau and the cylinder diameter so that params.reynolds() equals RE.\n"
              "--gpus N cuts the lattice into N row strips, one per GPU of this node, advanced in lockstep by this process\n"
              "with the halo rows copied GPU to GPU over xGMI (--rccl: RCCL send/recv instead); --strips M > N puts several\n"
              "strips on one GPU. --contracted: FMA-contracted collision (as the reference's -ffast-math -mfma build).\n"
              "--obstacle-mask: the obstacle as a P5 / P2 PGM of exactly nx x ny pixels (nonzero = solid; the first image row\n"
              "is the top lattice row) in place of the cylinder; Cd / Cl and the Reynolds number then use its frontal height.\n"
              "--obstacle-bodies: the same PGM with the grey value as the body number (0 fluid, 1..255; maxval above 255 is refused; not\n"
              "together with --obstacle-mask). Geometry, forces.csv and the Cd / Cl summary are those of the mask; forces_bodies.csv adds\n"
              "drag and lift per body (momentum exchange over the links that end in it), with the rows a body spans as its own D.\n"
              "--inlet-profile: one inlet velocity per row instead of the plug inflow. parabolic: the Poiseuille profile\n"
              "s(1-s), s = (y+0.5)/ny; FILE: a text file of ny numbers, row 0 (bottom) first ('#' comments and blank lines\n"
              "allowed), giving the shape. Either is scaled so that its mean over the ny rows is the inlet velocity, which\n"
              "stays the reference velocity: Reynolds number, --reynolds and Cd / Cl refer to the bulk (mean) velocity.\n"
              "--print-inlet-profile: print the ny inlet velocities (row 0 first) and exit without opening a device.\n"
              "--inlet-ramp N / --inlet-pulse A:P / --inlet-schedule FILE: a time-dependent inflow; the inlet velocity of every row is\n"
              "multiplied by one factor s(t) per iteration t (counted from the start of the run, across --restart). ramp: the N + 1\n"
              "factors 0.5 (1 - cos(pi k / N)), from rest to the full inflow, the last one held; pulse: the P factors\n"
              "1 + A sin(2 pi k / P), repeated; FILE: a text file of up to 1048576 numbers ('#' comments allowed), the last one held,\n"
              "or repeated with --inlet-schedule-repeat. The three exclude each other. Negative factors reverse the inflow. The\n"
              "velocity of moving walls is not scaled, and Reynolds number and Cd / Cl keep referring to the inlet velocity. A ramp\n"
              "should be long against L / c_s: accelerating the channel needs a pressure difference against the outlet's fixed density.\n"
              "--print-inlet-schedule: print the factors and exit without opening a device.\n"
              "--smagorinsky CS: Smagorinsky LES collision with constant CS in [0, 1] (0: plain BGK) instead of BGK, for\n"
              "higher Reynolds numbers at the same tau. tau, the Reynolds number and --reynolds keep referring to the\n"
              "molecular viscosity (tau - 0.5) / 3; the eddy viscosity of the model is added per cell.\n"
              "--trt-magic LAMBDA: two-relaxation-time (TRT) collision with magic parameter LAMBDA in [0, 1] (0: plain BGK)\n"
              "instead of BGK: the even part of each opposite pair of populations relaxes with 1/tau (the viscosity is\n"
              "unchanged), the odd part with 1/(0.5 + LAMBDA/(tau - 0.5)). 0.25 is the most stable choice, 0.1875 (3/16) the\n"
              "most accurate at walls. Needs tau > 0.5; cannot be combined with --smagorinsky.\n"
              "--forcing FX,FY: a uniform driving force density (FX, FY) in lattice units on every fluid cell and iteration (one token;\n"
              "either number may be negative, each of magnitude below 1): a pressure-gradient-equivalent drive, gravity, a cross-stream\n"
              "force. Guo's scheme on the BGK collision: the velocity of the equilibrium and of every output is (sum c f + F/2) / rho.\n"
              "A channel of H rows between the walls carries the parabola of peak u_max under FX = 8 nu u_max / H^2. The inlet, the outlet\n"
              "and the walls do not know about the force. Cannot be combined with --smagorinsky or --trt-magic.\n"
              "--mrt BULK,MAGIC: multiple-relaxation-time (MRT) collision (one token): TRT with magic parameter MAGIC in (0, 1] whose bulk\n"
              "rate BULK in (0, 2) is free of tau. The trace of the stress (the energy moments) relaxes with BULK, so the bulk viscosity\n"
              "grows with 1/BULK - 1/2 and pressure waves of an impulsive start die out; the shear viscosity stays (tau - 0.5) / 3.\n"
              "BULK = 1/tau is --trt-magic MAGIC; BULK 0: plain BGK. Needs tau > 0.5; cannot be combined with --smagorinsky, --trt-magic\n"
              "or --forcing.\n"
              "--sponge WIDTH:TAU_END: outlet sponge zone (one token): over the last WIDTH columns (1 .. nx-1) the relaxation time rises\n"
              "smoothly from tau to TAU_END > 0.5, tau_x = tau + (TAU_END - tau) s^2 with s the fraction of the zone behind the column, so\n"
              "that vortices and pressure waves are diffused before they meet the outlet, which reflects them. The viscosity inside the\n"
              "zone is (tau_x - 0.5) / 3: results taken there are not those of the fluid. WIDTH 0: none. Needs tau > 0.5; cannot be\n"
              "combined with --smagorinsky, --trt-magic, --forcing or --mrt.\n"
              "--wall-south KIND / --wall-north KIND: the bottom (row 0) / top (row ny-1) wall, KIND = no-slip (the default: on-node\n"
              "bounce-back) | free-slip (specular reflection: no boundary layer, for unconfined flow past a body) | moving:U (a wall\n"
              "sliding at the tangential velocity U, |U| < 1: Couette flow, a lid, a moving ground). --walls KIND sets both. The\n"
              "on-node scheme does not make ux on a moving wall's row equal U, and the wall's density is taken as 1.\n"
              "--inlet velocity|pressure:RHO / --outlet pressure:RHO|velocity:U: the two open ends, column 0 and column nx-1. The\n"
              "defaults are the reference's: a Zou-He velocity inlet (--inlet-velocity, --inlet-profile, the inlet schedules) and a Zou-He\n"
              "pressure outlet with RHO = 1. --inlet pressure:RHO gives the inlet's density (RHO > 0) and solves for its velocity;\n"
              "--outlet velocity:U gives the outlet's velocity (|U| < 1, positive leaves the domain: suction, a piston) and solves for\n"
              "its density. A channel driven from rest by a density difference: --inlet-velocity 0 --inlet pressure:1.005 --outlet\n"
              "pressure:0.995. A pressure inlet takes no --inlet-profile and no inlet schedule; Reynolds number and Cd / Cl keep\n"
              "referring to --inlet-velocity. The ports do not know about --forcing, and the on-node walls exchange mass with the fluid\n"
              "wherever the density is not 1, so the flux of a pressure-driven channel is not constant along x.\n"
              "--periodic-y: periodic top and bottom boundaries in place of the two walls: row -1 is row ny-1 and row ny is row 0, for the\n"
              "flow, the obstacle (a body may lie across the seam) and --inlet-profile; no wall rule runs. For a cascade or an infinite row\n"
              "of bodies, a wake without blockage, a shear layer, a cross-stream --forcing. Also with --gpus N / --strips N (every strip at\n"
              "least 12 rows). Not with a wall KIND other than no-slip, and not with --obstacle-bodies that touch row 0 or row ny-1.\n"
              "--stats-start N: time-averaged statistics from step N on, sampled on the device every --output-frequency steps;\n"
              "the run ends with mean_fields.vtk and mean_fields.csv (means of rho, ux, uy and the Reynolds stresses). With\n"
              "--checkpoint / --restart the sums travel beside the checkpoint as FILE.stats. --no-final suppresses the two\n"
              "mean_fields files like the other end-of-run fields (FILE.stats is still written with --checkpoint).\n"
              "--frame-stride K: at every output iteration the device averages rho, ux, uy and the vorticity d uy/dx - d ux/dy over\n"
              "K x K cells (1 <= K <= 64; K must divide nx, ny and the rows of every strip) and the frame is written as\n"
              "vtk_output/frame_%06d.vtk (STRUCTURED_POINTS, spacing K; vector velocity, scalars density and vorticity), also with\n"
              "--no-vtk: 4 nx ny / K^2 floats per frame leave the device instead of the full-resolution fields.\n"
              "--probes FILE: point probes, one `x y` per line in lattice coordinates (0 <= x <= nx-1, 0 <= y <= ny-1; '#' starts a\n"
              "comment). --probe-line x0 y0 x1 y1 n: n equally spaced probes from (x0, y0) to (x1, y1), end points included; may be\n"
              "repeated and combined with --probes (at most 65536 points in all, numbered in the order given). At every output\n"
              "iteration the device interpolates rho, ux, uy bilinearly at the probes and probes.csv gains one row per probe\n"
              "(timestep,probe,x,y,rho,ux,uy at %.17g); no field leaves the device for it.");
}

int main(int argc, char** argv) {
    LBM::SimulationParams params;
    LBM::BackendOptions opt;
    bool vtk = true, final_results = true;
    std::string restart_from, checkpoint_to;
    bool print_profile = false;
    bool print_schedule = false, schedule_repeat = false;
    std::string schedule_option, schedule_file;   // which of the three sources gave the schedule; the FILE of --inlet-schedule
    const char* smagorinsky = nullptr;
    const char* trt_magic = nullptr;
    const char* forcing = nullptr;
    const char* mrt = nullptr;
    const char* sponge = nullptr;
    const char* stats_start = nullptr;
    const char* frame_stride = nullptr;
    std::vector<LBM::ProbePoint> probe_points;
    bool probes_asked = false;
    double reynolds = -1.0;
    for (int a = 1; a < argc; ++a) {
        const std::string k = argv[a];
        auto val = [&]() -> const char* {
            if (a + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", k.c_str()); std::exit(2); }
            return argv[++a];
        };
        if (k == "--nx") params.nx = std::atoi(val());
        else if (k == "--ny") params.ny = std::atoi(val());
        else if (k == "--steps") params.num_timesteps = std::atoi(val());
        else if (k == "--output-frequency") params.output_frequency = std::atoi(val());
        else if (k == "--tau") params.tau = std::atof(val());
        else if (k == "--inlet-velocity") params.inlet_velocity = std::atof(val());
        else if (k == "--reynolds") reynolds = std::atof(val());
        else if (k == "--cylinder-x") params.cylinder_x = std::atof(val());
        else if (k == "--cylinder-y") params.cylinder_y = std::atof(val());
        else if (k == "--cylinder-radius") params.cylinder_radius = std::atof(val());
        else if (k == "--vtk-start-step") params.vtk_start_step = std::atoi(val());
        else if (k == "--no-vtk") vtk = false;
        else if (k == "--no-final") final_results = false;
        else if (k == "--sync-vtk") opt.async_vtk = false;
        else if (k == "--fp32") opt.fp32 = true;
        else if (k == "--no-tune") opt.tune = false;
        else if (k == "--contracted") opt.contracted = true;
        else if (k == "--gpus") opt.gpus = std::atoi(val());
        else if (k == "--strips") opt.strips = std::atoi(val());
        else if (k == "--rccl") opt.rccl = true;
        else if (k == "--device") opt.device = std::atoi(val());
        else if (k == "--quiet") opt.quiet = true;
        else if (k == "--restart") restart_from = val();
        else if (k == "--checkpoint") checkpoint_to = val();
        else if (k == "--obstacle-mask") params.obstacle_mask_file = val();
        else if (k == "--obstacle-bodies") params.obstacle_bodies_file = val();
        else if (k == "--inlet-profile") params.inlet_profile_spec = val();
        else if (k == "--print-inlet-profile") print_profile = true;
        else if (k == "--smagorinsky") smagorinsky = val();
        else if (k == "--trt-magic") trt_magic = val();
        else if (k == "--forcing") forcing = val();
        else if (k == "--mrt") mrt = val();
        else if (k == "--sponge") sponge = val();
        else if (k == "--stats-start") stats_start = val();
        else if (k == "--periodic-y") params.periodic_y = true;
        else if (k == "--wall-south" || k == "--wall-north" || k == "--walls") {   // checked here: no device is touched before a bad value exits
            try {
                const std::string kind = val();
                if (k != "--wall-north") params.set_wall(0, k, kind);
                if (k != "--wall-south") params.set_wall(1, k, kind);
            } catch (const std::exception& e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 2;
            }
        }
        else if (k == "--inlet" || k == "--outlet") {   // checked here: no device is touched before a bad value exits
            try {
                params.set_port(k == "--inlet" ? 0 : 1, k, val());
            } catch (const std::exception& e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 2;
            }
        }
        else if (k == "--inlet-ramp" || k == "--inlet-pulse" || k == "--inlet-schedule") {   // parsed here: no device is touched before a bad value exits
            try {
                const std::string text = val();
                if (!schedule_option.empty())
                    throw std::invalid_argument(k + " cannot be combined with " + schedule_option + " (one inlet schedule at a time)");
                schedule_option = k;
                if (k == "--inlet-ramp") { params.inlet_schedule = LBM::parse_inlet_ramp(text); params.inlet_schedule_spec = "ramp:" + text; }
                else if (k == "--inlet-pulse") { params.inlet_schedule = LBM::parse_inlet_pulse(text); params.inlet_schedule_spec = "pulse:" + text; params.inlet_schedule_mode = 1; }
                else { params.inlet_schedule = LBM::read_inlet_schedule(text); params.inlet_schedule_spec = schedule_file = text; }
            } catch (const std::exception& e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 2;
            }
        }
        else if (k == "--inlet-schedule-repeat") schedule_repeat = true;
        else if (k == "--print-inlet-schedule") print_schedule = true;
        else if (k == "--frame-stride") frame_stride = val();
        else if (k == "--probes" || k == "--probe-line") {   // parsed here, in the order given; checked against the lattice below
            try {
                std::vector<LBM::ProbePoint> more;
                if (k == "--probes") more = LBM::read_probe_file(val());
                else {
                    if (a + 5 >= argc) { std::fprintf(stderr, "--probe-line takes five values: x0 y0 x1 y1 n\n"); return 2; }
                    more = LBM::parse_probe_line(argv + a + 1);
                    a += 5;
                }
                probe_points.insert(probe_points.end(), more.begin(), more.end());
                probes_asked = true;
            } catch (const std::exception& e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 2;
            }
        }
        else if (k == "--help" || k == "-h") { usage(); return 0; }
        else { std::fprintf(stderr, "unknown option %s\n", k.c_str()); usage(); return 2; }
    }
    if (smagorinsky) {   // checked before any device is touched: a whole finite number in [0, 1]
        char* end = nullptr;
        const double cs = std::strtod(smagorinsky, &end);
        if (end == smagorinsky || *end != '\0' || !std::isfinite(cs) || cs < 0.0 || cs > 1.0) {
            std::fprintf(stderr, "--smagorinsky: '%s' is not a number in [0, 1]\n", smagorinsky);
            return 2;
        }
        params.smagorinsky_cs = cs;
    }
    if (trt_magic) {     // likewise: a whole finite number in [0, 1], a tau it is defined for, and no second collision model
        char* end = nullptr;
        const double magic = std::strtod(trt_magic, &end);
        if (end == trt_magic || *end != '\0' || !std::isfinite(magic) || magic < 0.0 || magic > 1.0) {
            std::fprintf(stderr, "--trt-magic: '%s' is not a number in [0, 1]\n", trt_magic);
            return 2;
        }
        if (magic > 0.0 && !(params.tau > 0.5)) {
            std::fprintf(stderr, "--trt-magic: needs tau > 0.5, not %g\n", params.tau);
            return 2;
        }
        if (magic > 0.0 && params.smagorinsky_cs > 0.0) {
            std::fprintf(stderr, "--trt-magic cannot be combined with --smagorinsky (one collision model at a time)\n");
            return 2;
        }
        params.trt_magic = magic;
    }
    if (forcing) {       // likewise: FX,FY parsed whole, and no second collision model
        try {
            params.set_forcing(forcing);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
        if (params.forced() && (params.smagorinsky_cs > 0.0 || params.trt_magic > 0.0)) {
            std::fprintf(stderr, "--forcing cannot be combined with %s (one collision model at a time)\n", params.smagorinsky_cs > 0.0 ? "--smagorinsky" : "--trt-magic");
            return 2;
        }
    }
    if (mrt) {           // likewise: BULK,MAGIC parsed whole, a tau the rates are defined for, and no second collision model (in the words of
                         // the library's setters, set_collision in csrc/lbm_hip.hip, which a context would meet after a device is open)
        try {
            params.set_mrt(mrt);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
        if (params.mrt() && !(params.tau > 0.5)) {
            std::fprintf(stderr, "--mrt: tau = %g (the MRT rates need tau > 0.5)\n", params.tau);
            return 2;
        }
        char other[160] = "";
        if (params.smagorinsky_cs > 0.0) std::snprintf(other, sizeof(other), "Smagorinsky constant Cs = %g", params.smagorinsky_cs);
        else if (params.trt_magic > 0.0) std::snprintf(other, sizeof(other), "TRT magic parameter %g", params.trt_magic);
        else if (params.forced()) std::snprintf(other, sizeof(other), "forcing F = (%g, %g)", params.forcing_x, params.forcing_y);
        if (params.mrt() && other[0]) {
            std::fprintf(stderr, "--mrt: (bulk rate, magic) = (%g, %g) on a context with %s (the two collisions cannot be combined)\n", params.mrt_bulk_rate, params.mrt_magic, other);
            return 2;
        }
    }
    if (sponge) {        // likewise: WIDTH:TAU_END parsed whole, a width the grid holds, a tau the rates are defined for, and no second
                         // collision model (in the words of the library's setters)
        try {
            params.set_sponge(sponge);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
        if (params.sponge_width > params.nx - 1) {
            std::fprintf(stderr, "--sponge: width = %d (0 .. nx - 1 = %d only: column 0 keeps tau)\n", params.sponge_width, params.nx - 1);
            return 2;
        }
        if (params.sponge() && !(params.tau > 0.5)) {
            std::fprintf(stderr, "--sponge: tau = %g (the sponge's rates need tau > 0.5)\n", params.tau);
            return 2;
        }
        char other[160] = "";
        if (params.smagorinsky_cs > 0.0) std::snprintf(other, sizeof(other), "Smagorinsky constant Cs = %g", params.smagorinsky_cs);
        else if (params.trt_magic > 0.0) std::snprintf(other, sizeof(other), "TRT magic parameter %g", params.trt_magic);
        else if (params.forced()) std::snprintf(other, sizeof(other), "forcing F = (%g, %g)", params.forcing_x, params.forcing_y);
        else if (params.mrt()) std::snprintf(other, sizeof(other), "MRT parameters (bulk rate, magic) = (%g, %g)", params.mrt_bulk_rate, params.mrt_magic);
        if (params.sponge() && other[0]) {
            std::fprintf(stderr, "--sponge: (width, tau_end) = (%d, %g) on a context with %s (the two collisions cannot be combined)\n", params.sponge_width, params.sponge_tau_end, other);
            return 2;
        }
    }
    if (stats_start) {   // checked before any device is touched: a whole number >= 0, and a cadence to sample at
        char* end = nullptr;
        const long n = std::strtol(stats_start, &end, 10);
        if (end == stats_start || *end != '\0' || n < 0 || n > 2147483647L) {
            std::fprintf(stderr, "--stats-start: '%s' is not a step number >= 0\n", stats_start);
            return 2;
        }
        if (params.output_frequency <= 0) {
            std::fprintf(stderr, "--stats-start needs --output-frequency > 0: statistics are sampled at the output cadence\n");
            return 2;
        }
        params.stats_start = (int)n;
    }
    if (frame_stride) {   // checked before any device is touched: a whole number in 1..64 that divides nx and every strip's rows
        char* end = nullptr;
        const long K = std::strtol(frame_stride, &end, 10);
        if (end == frame_stride || *end != '\0' || K < 1 || K > 64) {
            std::fprintf(stderr, "--frame-stride: '%s' is not a whole number in 1..64\n", frame_stride);
            return 2;
        }
        if (params.output_frequency <= 0) {
            std::fprintf(stderr, "--frame-stride needs --output-frequency > 0: frames are written at the output cadence\n");
            return 2;
        }
        if (params.nx < 2 || params.ny < 2 || params.nx % K != 0 || params.ny % K != 0) {
            std::fprintf(stderr, "--frame-stride: %ld does not divide the lattice %dx%d\n", K, params.nx, params.ny);
            return 2;
        }
        // the row strips as Grid cuts them (the first ny % n strips get one more row)
        const int nstrips = std::min(params.ny, opt.strips > 0 ? opt.strips : std::max(1, opt.gpus));
        for (int s = 0, y = 0; s < nstrips; ++s) {
            const int rows = params.ny / nstrips + (s < params.ny % nstrips ? 1 : 0);
            if (y % K != 0 || rows % K != 0) {
                std::fprintf(stderr, "--frame-stride: %ld does not divide the rows of strip %d of %d (rows %d..%d)\n", K, s, nstrips, y, y + rows - 1);
                return 2;
            }
            y += rows;
        }
        params.frame_stride = (int)K;
    }
    if (probes_asked) {   // checked before any device is touched: points inside the lattice, and a cadence to sample at
        if (params.output_frequency <= 0) {
            std::fprintf(stderr, "--probes / --probe-line need --output-frequency > 0: probes are sampled at the output cadence\n");
            return 2;
        }
        try {
            LBM::check_probe_points(probe_points, params.nx, params.ny);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
        for (const LBM::ProbePoint& p : probe_points) { params.probe_xy.push_back(p.x); params.probe_xy.push_back(p.y); }
    }
    if (!params.obstacle_bodies_file.empty() && !params.obstacle_mask_file.empty()) {
        std::fprintf(stderr, "--obstacle-bodies and --obstacle-mask exclude each other: the labels are the mask\n");
        return 2;
    }
    if (!params.obstacle_bodies_file.empty()) {   // parsed and checked before any device is touched, like the mask
        try {
            LBM::ObstacleMask m = LBM::read_obstacle_pgm(params.obstacle_bodies_file, params.nx, params.ny, "--obstacle-bodies", true);
            params.obstacle_mask = std::move(m.cells);
            params.mask_frontal_height = m.frontal_height;
            params.body_cells = std::move(m.body_cells);
            params.body_height = std::move(m.body_height);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    if (!params.obstacle_mask_file.empty()) {   // parsed and checked before any device is touched
        try {
            LBM::ObstacleMask m = LBM::read_obstacle_pgm(params.obstacle_mask_file, params.nx, params.ny);
            params.obstacle_mask = std::move(m.cells);
            params.mask_frontal_height = m.frontal_height;
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    if (params.periodic_y) {   // checked before any device is touched: what lbm_initialise would refuse
        if (params.walled()) {
            std::fprintf(stderr, "--periodic-y cannot be combined with a %s wall (--wall-south / --wall-north / --walls): no wall rule runs on a periodic lattice\n",
                         params.wall_text(params.wall_kind[0] != 0 ? 0 : 1).c_str());
            return 2;
        }
        const int nstrips = std::min(params.ny, opt.strips > 0 ? opt.strips : std::max(1, opt.gpus));
        if (params.ny / std::max(1, nstrips) < 12) {
            std::fprintf(stderr, "--periodic-y: %d rows in %d strip(s): every strip needs at least 12 rows\n", params.ny, nstrips);
            return 2;
        }
        if (params.bodied())
            for (int row : {0, params.ny - 1})
                for (int x = 0; x < params.nx; ++x)
                    if (params.obstacle_mask[(size_t)row * params.nx + x]) {
                        std::fprintf(stderr, "--periodic-y: --obstacle-bodies has a labelled cell on row %d: a body's links across the seam would be missed (keep bodies off rows 0 and %d, or use --obstacle-mask)\n",
                                     row, params.ny - 1);
                        return 2;
                    }
    }
    if (reynolds > 0.0 && params.masked()) params.inlet_velocity = reynolds * params.nu() / params.mask_frontal_height;
    else if (reynolds > 0.0) params.inlet_velocity = reynolds * params.nu() / (2.0 * params.cylinder_radius * params.ny);
    if (!params.inlet_profile_spec.empty()) {   // scaled to the final inlet velocity, checked before any device is touched
        try {
            params.inlet_profile = LBM::build_inlet_profile(params.inlet_profile_spec, params.ny, params.inlet_velocity);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    if (params.port_kind[0] == 1 && (!params.inlet_profile_spec.empty() || params.scheduled())) {   // a pressure inlet solves for its velocity
        std::fprintf(stderr, "--inlet pressure:RHO cannot be combined with %s: a pressure inlet takes no inlet velocity\n",
                     !params.inlet_profile_spec.empty() ? "--inlet-profile" : schedule_option.c_str());
        return 2;
    }
    if (print_profile) {
        if (!params.profiled()) { std::fprintf(stderr, "--print-inlet-profile needs --inlet-profile\n"); return 2; }
        for (double u : params.inlet_profile) std::printf("%.17g\n", u);
        return 0;
    }
    if (schedule_repeat) {   // the mode of --inlet-schedule FILE alone: a ramp holds and a pulse repeats by what they are
        if (schedule_file.empty()) { std::fprintf(stderr, "--inlet-schedule-repeat needs --inlet-schedule FILE\n"); return 2; }
        params.inlet_schedule_mode = 1;
        params.inlet_schedule_spec += ":repeat";
    }
    if (print_schedule) {
        if (!params.scheduled()) { std::fprintf(stderr, "--print-inlet-schedule needs --inlet-ramp, --inlet-pulse or --inlet-schedule\n"); return 2; }
        for (double s : params.inlet_schedule) std::printf("%.17g\n", s);
        return 0;
    }
    if (params.scheduled()) {   // against the final inlet velocities, checked before any device is touched: the inlet divides by 1 - u s
        try {
            LBM::check_inlet_schedule(params.profiled() ? params.inlet_profile : std::vector<double>(1, params.inlet_velocity), params.inlet_schedule);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    try {
        LBM::Solver solver(params, vtk, opt);
        LBM::IOManager io_manager;
        solver.initialise();
        if (!restart_from.empty()) solver.load_state(restart_from);   // continues at the saved iteration
        const bool success = solver.run(io_manager);
        if (success && !checkpoint_to.empty()) solver.save_state(checkpoint_to);
        if (success) {
            if (final_results) io_manager.write_final_results(solver.get_grid(), solver.get_params());
            if (final_results && params.stats()) LBM::IOManager::write_mean_fields(solver.get_grid().stat_sums(), solver.get_grid().stats_samples(), solver.get_params());
            std::printf("\nSimulation completed successfully!\n");
        } else {
            std::fprintf(stderr, "LBM simulation failed.\n");
            return 1;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "An exception occurred: %s\n", e.what());
        return 1;
    }
    return 0;
}
