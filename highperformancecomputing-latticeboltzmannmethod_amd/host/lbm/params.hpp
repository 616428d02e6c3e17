// host/lbm/params.hpp — lattice constants and run parameters of the solver surface.
// Mirrors /root/reference/include/LBMConfig.h (names, field order, defaults and derived quantities are the public
// surface a caller of the reference touches: LBMConfig.h:9-34 constants, :36-66 SimulationParams).
#pragma once
#include <array>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

namespace LBM {

inline constexpr int Q = 9;   // LBMConfig.h:9
inline constexpr int D = 2;   // LBMConfig.h:10

// Direction numbering 0:(0,0) 1:E 2:N 3:W 4:S 5:NE 6:NW 7:SW 8:SE — observable through f_current(x,y,i).
inline constexpr std::array<std::array<int, 2>, Q> VELOCITIES = {{
    {{0, 0}}, {{1, 0}}, {{0, 1}}, {{-1, 0}}, {{0, -1}}, {{1, 1}}, {{-1, 1}}, {{-1, -1}}, {{1, -1}}}};
inline constexpr std::array<double, Q> WEIGHTS = {4.0 / 9.0,  1.0 / 9.0,  1.0 / 9.0,  1.0 / 9.0, 1.0 / 9.0,
                                                 1.0 / 36.0, 1.0 / 36.0, 1.0 / 36.0, 1.0 / 36.0};
inline constexpr std::array<int, Q> OPPOSITE = {0, 3, 4, 1, 2, 7, 8, 5, 6};

struct SimulationParams {
    double tau = 0.6;
    double inlet_velocity = 0.01333;
    int nx = 2048;
    int ny = 512;
    int num_timesteps = 120000;
    int output_frequency = 140;
    double cylinder_x = 0.2;        // fraction of nx
    double cylinder_y = 0.5;        // fraction of ny
    double cylinder_radius = 0.05;  // fraction of ny
    int vtk_start_step = 0;
    // user-defined obstacle (lbm_solver --obstacle-mask; not in the reference): the global [ny][nx] mask, row 0 first, in place of
    // the cylinder. Its reference length D is the frontal height: the number of rows that hold a solid cell.
    std::string obstacle_mask_file;
    std::vector<unsigned char> obstacle_mask;
    int mask_frontal_height = 0;
    // per-body forces (lbm_solver --obstacle-bodies; not in the reference): the same geometry from a PGM whose grey value is the body
    // number; obstacle_mask then holds the labels (nonzero = solid, as lbm_set_body_labels reads them). Per body 1..B: its cells and
    // the rows it spans, the D of its own coefficients in forces_bodies.csv. Everything a masked run writes stays as it is.
    std::string obstacle_bodies_file;
    std::vector<int> body_cells, body_height;
    // per-row inlet profile (lbm_solver --inlet-profile; not in the reference): "parabolic" or the file of its shape, and the ny
    // absolute velocities, row 0 first, whose mean is inlet_velocity (host/lbm/inlet.hpp). Empty: inlet_velocity on every row.
    std::string inlet_profile_spec;
    std::vector<double> inlet_profile;
    // inlet schedule (lbm_solver --inlet-ramp N | --inlet-pulse A:P | --inlet-schedule FILE [--inlet-schedule-repeat]; not in the
    // reference, whose inflow is frozen): how it was asked for ("ramp:N", "pulse:A:P", "FILE" or "FILE:repeat"), the scale factor of
    // the inflow per iteration and the mode (0 hold the last entry, 1 repeat) as lbm_set_inlet_schedule takes them (host/lbm/inlet.hpp).
    // Empty: the frozen inflow. The moving walls' velocity is not scaled, and Cd / Cl keep referring to inlet_velocity.
    std::string inlet_schedule_spec;
    std::vector<double> inlet_schedule;
    int inlet_schedule_mode = 0;
    // Smagorinsky LES collision (lbm_solver --smagorinsky; not in the reference): the constant Cs, 0 = plain BGK. tau, nu() and
    // reynolds() keep referring to the molecular viscosity.
    double smagorinsky_cs = 0.0;
    // Two-relaxation-time collision (lbm_solver --trt-magic; not in the reference): the magic parameter, 0 = plain BGK. Never
    // together with smagorinsky_cs. tau keeps setting the viscosity.
    double trt_magic = 0.0;
    // Uniform driving force (lbm_solver --forcing FX,FY; not in the reference): a constant force density in lattice units on every
    // fluid cell, Guo's scheme on the BGK collision (lbm_set_forcing). (0, 0) = none. Never together with smagorinsky_cs or trt_magic.
    double forcing_x = 0.0, forcing_y = 0.0;
    // Multiple-relaxation-time collision (lbm_solver --mrt BULK,MAGIC; not in the reference): TRT with the magic parameter MAGIC whose
    // bulk rate BULK, in (0, 2), is free of tau (lbm_set_mrt). Bulk rate 0 = plain BGK. Never together with smagorinsky_cs, trt_magic
    // or a force. tau keeps setting the shear viscosity.
    double mrt_bulk_rate = 0.0, mrt_magic = 0.0;
    // Outlet sponge zone (lbm_solver --sponge WIDTH:TAU_END; not in the reference): over the last WIDTH columns the relaxation time rises
    // from tau to TAU_END (lbm_set_sponge). Width 0 = none. Never together with smagorinsky_cs, trt_magic, a force or MRT.
    int sponge_width = 0;
    double sponge_tau_end = 0.0;
    // time-averaged statistics (lbm_solver --stats-start; not in the reference): the first step sampled, -1 = off. Samples are taken on
    // the device at the output_frequency cadence (lbm_stats_begin); the run ends with mean_fields.vtk / mean_fields.csv.
    int stats_start = -1;
    // coarsened flow frames (lbm_solver --frame-stride; not in the reference): the stride K of the k x k block averages, 0 = off. One
    // frame (rho, ux, uy, vorticity) is written on the device at every output iteration (lbm_frames_begin) and drained into
    // vtk_output/frame_%06d.vtk; the full-resolution fields are not fetched for it.
    int frame_stride = 0;
    // point probes (lbm_solver --probes / --probe-line; not in the reference): [n][2] points (x, y) in global lattice coordinates, empty =
    // off. (rho, ux, uy) is sampled at them on the device at every output iteration, bilinearly (lbm_probes_begin), and drained into
    // probes.csv; no field is fetched for it.
    std::vector<double> probe_xy;
    // the bottom and top walls (lbm_solver --wall-south / --wall-north / --walls; not in the reference, whose two walls are no-slip):
    // [0] south (row 0), [1] north (row ny - 1); kind 0 no-slip, 1 free-slip, 2 moving with the tangential velocity beside it
    // (lbm_set_wall). Both no-slip: everything the run prints and writes is the reference's.
    int wall_kind[2] = {0, 0};
    double wall_velocity[2] = {0.0, 0.0};
    // the two open ends (lbm_solver --inlet / --outlet; not in the reference, whose pair is a velocity inlet and a pressure outlet
    // with rho = 1): [0] west (column 0), [1] east (column nx - 1); kind 0 velocity, 1 pressure, with the density of a pressure port
    // or the velocity of the east velocity port beside it (lbm_set_port). The defaults: everything the run prints and writes is the
    // reference's.
    int port_kind[2] = {0, 1};
    double port_value[2] = {0.0, 1.0};
    // periodic top and bottom boundaries (lbm_solver --periodic-y; not in the reference, whose rows 0 and ny - 1 are walls): row -1 is
    // row ny - 1 and row ny is row 0, for the populations, the geometry and the inlet profile; no wall rule runs (lbm_set_periodic_y).
    // Off: everything the run prints and writes is the reference's.
    bool periodic_y = false;

    double nu() const { return (tau - 0.5) / 3.0; }
    bool masked() const { return !obstacle_mask.empty(); }
    bool bodied() const { return !obstacle_bodies_file.empty(); }
    int body_count() const { return (int)body_height.size(); }
    bool profiled() const { return !inlet_profile.empty(); }
    bool scheduled() const { return !inlet_schedule.empty(); }
    bool les() const { return smagorinsky_cs > 0.0; }
    bool trt() const { return trt_magic > 0.0; }
    bool forced() const { return forcing_x != 0.0 || forcing_y != 0.0; }
    bool mrt() const { return mrt_bulk_rate != 0.0; }
    bool sponge() const { return sponge_width > 0; }
    bool stats() const { return stats_start >= 0; }
    bool frames() const { return frame_stride > 0; }
    bool probes() const { return !probe_xy.empty(); }
    int probe_count() const { return (int)(probe_xy.size() / 2); }
    bool walled() const { return wall_kind[0] != 0 || wall_kind[1] != 0; }
    bool ported() const { return port_kind[0] != 0 || port_kind[1] != 1 || port_value[1] != 1.0; }
    // a number with the fewest digits that read back exactly (csrc/lbm_ckpt.hpp holds a copy for the ports in a checkpoint's refusal: the
    // library does not include this layer; the two must stay alike, so that a port reads the same in simulation_params.csv and there)
    static std::string shortest_text(double v) {
        char b[64];
        for (int digits = 1; digits <= 17; ++digits) {
            std::snprintf(b, sizeof(b), "%.*g", digits, v);
            if (std::strtod(b, nullptr) == v) break;
        }
        return b;
    }
    // the velocity of wall `side` in that form
    std::string wall_velocity_text(int side) const { return shortest_text(wall_velocity[side]); }
    // FX,FY of --forcing: one token, two finite numbers of magnitude below 1, each parsed whole (std::invalid_argument with the one-line
    // message otherwise)
    void set_forcing(const std::string& text) {
        const auto bad = [&](const char* why) {
            return std::invalid_argument("--forcing: '" + text + "' " + why + " (FX,FY: two numbers of magnitude below 1)");
        };
        const size_t comma = text.find(',');
        if (comma == std::string::npos || text.find(',', comma + 1) != std::string::npos) throw bad("is not a pair FX,FY");
        const std::string part[2] = {text.substr(0, comma), text.substr(comma + 1)};
        double v[2];
        for (int k = 0; k < 2; ++k) {
            char* end = nullptr;
            v[k] = std::strtod(part[k].c_str(), &end);
            if (part[k].empty() || std::isspace((unsigned char)part[k][0]) || end == part[k].c_str() || *end != '\0') throw bad(k ? "has no number FY" : "has no number FX");
            if (!std::isfinite(v[k]) || std::fabs(v[k]) >= 1.0) throw bad("has a component that is not finite or not below 1 in magnitude");
        }
        forcing_x = v[0]; forcing_y = v[1];
    }
    // BULK,MAGIC of --mrt: one token, two numbers each parsed whole, BULK 0 or in (0, 2), MAGIC in (0, 1] beside a nonzero BULK
    // (std::invalid_argument with the one-line message otherwise)
    void set_mrt(const std::string& text) {
        const auto bad = [&](const char* why) {
            return std::invalid_argument("--mrt: '" + text + "' " + why + " (BULK,MAGIC: the bulk rate, 0 or in (0, 2), and the magic parameter in (0, 1])");
        };
        const size_t comma = text.find(',');
        if (comma == std::string::npos || text.find(',', comma + 1) != std::string::npos) throw bad("is not a pair BULK,MAGIC");
        const std::string part[2] = {text.substr(0, comma), text.substr(comma + 1)};
        double v[2];
        for (int k = 0; k < 2; ++k) {
            char* end = nullptr;
            v[k] = std::strtod(part[k].c_str(), &end);
            if (part[k].empty() || std::isspace((unsigned char)part[k][0]) || end == part[k].c_str() || *end != '\0') throw bad(k ? "has no number MAGIC" : "has no number BULK");
            if (!std::isfinite(v[k])) throw bad("has a number that is not finite");
        }
        if (v[0] < 0.0 || v[0] >= 2.0) throw bad("has a bulk rate outside (0, 2)");
        if (v[0] != 0.0 && (!(v[1] > 0.0) || v[1] > 1.0)) throw bad("has a magic parameter outside (0, 1]");
        mrt_bulk_rate = v[0]; mrt_magic = v[0] != 0.0 ? v[1] : 0.0;
    }
    // WIDTH:TAU_END of --sponge: one token, a whole number >= 0 and a number parsed whole, TAU_END finite and above 0.5 beside a nonzero
    // WIDTH (std::invalid_argument with the one-line message otherwise; the grid's bound on WIDTH is the caller's to check)
    void set_sponge(const std::string& text) {
        const auto bad = [&](const char* why) {
            return std::invalid_argument("--sponge: '" + text + "' " + why + " (WIDTH:TAU_END: the columns of the zone, 0 .. nx - 1, and the relaxation time at the outlet, above 0.5)");
        };
        const size_t colon = text.find(':');
        if (colon == std::string::npos || text.find(':', colon + 1) != std::string::npos) throw bad("is not a pair WIDTH:TAU_END");
        const std::string part[2] = {text.substr(0, colon), text.substr(colon + 1)};
        char* end = nullptr;
        const long w = std::strtol(part[0].c_str(), &end, 10);
        if (part[0].empty() || std::isspace((unsigned char)part[0][0]) || end == part[0].c_str() || *end != '\0') throw bad("has no whole number WIDTH");
        if (w < 0 || w > 2147483647L) throw bad("has a width below 0 or beyond any grid");
        const double t = std::strtod(part[1].c_str(), &end);
        if (part[1].empty() || std::isspace((unsigned char)part[1][0]) || end == part[1].c_str() || *end != '\0') throw bad("has no number TAU_END");
        if (w != 0 && (!std::isfinite(t) || !(t > 0.5))) throw bad("has a TAU_END that is not a finite number above 0.5");
        sponge_width = (int)w; sponge_tau_end = w != 0 ? t : 0.0;
    }
    // a wall as the command line names it: "no-slip", "free-slip" or "moving:U"
    std::string wall_text(int side) const {
        if (wall_kind[side] == 0) return "no-slip";
        if (wall_kind[side] == 1) return "free-slip";
        return "moving:" + wall_velocity_text(side);
    }
    // ... and as the banner prints it: "no-slip", "free-slip" or "moving u = U"
    std::string wall_banner(int side) const {
        return wall_kind[side] == 2 ? "moving u = " + wall_velocity_text(side) : wall_text(side);
    }
    // KIND of --wall-south / --wall-north / --walls into wall `side`: no-slip | free-slip | moving:U with a finite |U| < 1
    // (std::invalid_argument with the one-line message otherwise)
    void set_wall(int side, const std::string& option, const std::string& text) {
        const auto bad = [&](const char* why) {
            return std::invalid_argument(option + ": '" + text + "' " + why + " (no-slip, free-slip or moving:U with |U| < 1)");
        };
        if (text == "no-slip") { wall_kind[side] = 0; wall_velocity[side] = 0.0; return; }
        if (text == "free-slip") { wall_kind[side] = 1; wall_velocity[side] = 0.0; return; }
        if (text.rfind("moving:", 0) != 0) throw bad("is not a wall kind");
        const char* num = text.c_str() + 7;
        char* end = nullptr;
        const double u = std::strtod(num, &end);
        if (end == num || *end != '\0') throw bad("has no wall velocity");
        if (!std::isfinite(u) || std::fabs(u) >= 1.0) throw bad("has a wall velocity that is not finite or not below 1 in magnitude");
        wall_kind[side] = 2; wall_velocity[side] = u;
    }
    // a port as the command line names it: "velocity" (west), "velocity:U" (east) or "pressure:RHO"
    std::string port_text(int side) const {
        if (port_kind[side] == 1) return "pressure:" + shortest_text(port_value[side]);
        return side == 0 ? "velocity" : "velocity:" + shortest_text(port_value[side]);
    }
    // KIND of --inlet (side 0: velocity | pressure:RHO) / --outlet (side 1: pressure:RHO | velocity:U) with a finite RHO > 0 and a
    // finite |U| < 1 (std::invalid_argument with the one-line message otherwise)
    void set_port(int side, const std::string& option, const std::string& text) {
        const char* forms = side == 0 ? " (velocity or pressure:RHO with RHO > 0)" : " (pressure:RHO with RHO > 0 or velocity:U with |U| < 1)";
        const auto bad = [&](const char* why) { return std::invalid_argument(option + ": '" + text + "' " + why + forms); };
        if (side == 0 && text == "velocity") { port_kind[0] = 0; port_value[0] = 0.0; return; }
        const bool pressure = text.rfind("pressure:", 0) == 0, velocity = side == 1 && text.rfind("velocity:", 0) == 0;
        if (!pressure && !velocity) throw bad("is not a port kind");
        const char* num = text.c_str() + 9;
        char* end = nullptr;
        const double v = std::strtod(num, &end);
        if (end == num || *end != '\0' || std::isspace((unsigned char)*num)) throw bad(pressure ? "has no density" : "has no velocity");
        if (pressure && !(std::isfinite(v) && v > 0.0)) throw bad("has a density that is not finite or not above 0");
        if (velocity && !(std::isfinite(v) && std::fabs(v) < 1.0)) throw bad("has a velocity that is not finite or not below 1 in magnitude");
        port_kind[side] = pressure ? 1 : 0; port_value[side] = v;
    }
    double reynolds() const {
        if (masked()) return inlet_velocity * mask_frontal_height / nu();
        return inlet_velocity * (2.0 * cylinder_radius * ny) / nu();
    }
    int get_cylinder_x() const { return static_cast<int>(cylinder_x * nx); }
    int get_cylinder_y() const { return static_cast<int>(cylinder_y * ny); }
    int get_cylinder_radius_cells() const { return static_cast<int>(cylinder_radius * ny); }
};

// Build-side run options that the reference does not have (it hard-codes everything in main.cpp:11-12).
struct BackendOptions {
    int device = 0;               // first device; strip k runs on device (device + k) % visible devices ...
    int gpus = 1;                 // ... of the `gpus` devices used (clamped to the devices present)
    int strips = 0;               // row strips the lattice is cut into (0: one per GPU); > gpus: several strips share a GPU
    bool rccl = false;            // strip halos through RCCL (one communicator per strip; needs strips == gpus) instead of
                                  // peer copies over xGMI
    bool contracted = false;      // collision arithmetic: FMA-contracted + one reciprocal (lbm_set_option "arith" 1)
    bool fp32 = false;            // single-precision populations (build-only variant)
    bool tune = true;             // measured plan at initialise (lbm_set_option "tune")
    bool async_vtk = true;        // write VTK frames on a writer thread
    bool quiet = false;
};

}  // namespace LBM
