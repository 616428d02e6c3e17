// host/lbm/solver.hpp — LBM::Solver: constructor, initialise(), run(IOManager&), get_grid(), get_params() as in the
// reference (LBMSolver.h:23,31,43,80-81) plus step(t, io) = the loop body (LBMSolver.h:49-75), over the HIP backend.
#pragma once
#include "grid.hpp"
#include "io.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <sys/stat.h>

namespace LBM {

class Solver {
public:
    explicit Solver(const SimulationParams& params, bool enable_vtk = false, const BackendOptions& opt = {})
        : params_(params), opt_(opt), grid_(params, opt), enable_vtk_output_(enable_vtk) {
        if (enable_vtk || params.frames()) mkdir("vtk_output", 0755);   // LBMSolver.h:26-28
    }

    void initialise() {   // LBMSolver.h:31-41
        if (!opt_.quiet)
            std::printf("Cylinder Flow LBM Parameters:\n  Domain: %d×%d\n  tau = %g, nu = %g\n  Inlet velocity = %g\n"
                        "  Reynolds number = %g\n", params_.nx, params_.ny, params_.tau, params_.nu(),
                        params_.inlet_velocity, params_.reynolds());
        const int solid = grid_.setup_and_initialise();
        if (params_.stats()) {
            grid_.stats_begin(params_.stats_start);
            if (!opt_.quiet)
                std::printf("  Statistics: time averages from step %d on, one sample every %d steps\n", params_.stats_start, params_.output_frequency);
        }
        if (params_.frames()) {      // (two frames per chunk of run(): iterations 0 and output_frequency fall into the first one)
            grid_.frames_begin(params_.frame_stride, 4);
            if (!opt_.quiet)
                std::printf("  Frames: rho, u and vorticity averaged over %dx%d cells, one every %d steps (vtk_output/frame_*.vtk)\n", params_.frame_stride,
                            params_.frame_stride, params_.output_frequency);
        }
        if (params_.probes()) {      // (two samples per chunk of run(), like the frames)
            grid_.probes_begin(params_.probe_xy, 4);
            if (!opt_.quiet)
                std::printf("  Probes: rho and u at %d points, one sample every %d steps (probes.csv)\n", params_.probe_count(), params_.output_frequency);
        }
        if (!opt_.quiet && params_.profiled())
            std::printf("  Inlet: profile %s, mean velocity %g (Cd / Cl refer to it)\n", params_.inlet_profile_spec.c_str(), params_.inlet_velocity);
        if (!opt_.quiet && params_.scheduled())
            std::printf("  Inlet: schedule %s, %d factors, %s (the inflow of iteration t is scaled by s(t); the walls are not; Cd / Cl refer to the inlet velocity %g)\n",
                        params_.inlet_schedule_spec.c_str(), (int)params_.inlet_schedule.size(),
                        params_.inlet_schedule_mode ? "repeated" : "the last one holds", params_.inlet_velocity);
        if (!opt_.quiet && params_.les())
            std::printf("  Collision: Smagorinsky LES, Cs = %g (tau and the Reynolds number refer to the molecular viscosity)\n",
                        params_.smagorinsky_cs);
        if (!opt_.quiet && params_.trt())
            std::printf("  Collision: TRT collision, magic = %g (odd parts relax with 1/(0.5 + magic/(tau - 0.5)); tau sets the viscosity)\n",
                        params_.trt_magic);
        if (!opt_.quiet && params_.forced())
            std::printf("  driving force (Guo): Fx = %s, Fy = %s\n", SimulationParams::shortest_text(params_.forcing_x).c_str(),
                        SimulationParams::shortest_text(params_.forcing_y).c_str());
        if (!opt_.quiet && params_.mrt())
            std::printf("  Collision: MRT collision, bulk rate = %s, magic = %s (the trace of the stress relaxes with the bulk rate; tau sets the shear viscosity)\n",
                        SimulationParams::shortest_text(params_.mrt_bulk_rate).c_str(), SimulationParams::shortest_text(params_.mrt_magic).c_str());
        if (!opt_.quiet && params_.sponge())
            std::printf("  Outlet sponge: the last %d columns, tau rising to %s at the outlet (the viscosity there is (tau_x - 0.5) / 3)\n", params_.sponge_width,
                        SimulationParams::shortest_text(params_.sponge_tau_end).c_str());
        if (!opt_.quiet && params_.walled())
            std::printf("  Walls: south %s, north %s\n", params_.wall_banner(0).c_str(), params_.wall_banner(1).c_str());
        if (!opt_.quiet && params_.ported())
            std::printf("  Ports: inlet %s, outlet %s\n", params_.port_text(0).c_str(), params_.port_text(1).c_str());
        if (!opt_.quiet && params_.periodic_y)
            std::printf("  Top and bottom: periodic (row -1 is row %d; no wall rule runs)\n", params_.ny - 1);
        if (!opt_.quiet && params_.masked()) {
            std::printf("  Obstacle: %s %s, frontal height D=%d cells\n  Solid cells: %d\n  Plan: %s\n", params_.bodied() ? "bodies" : "mask",
                        params_.bodied() ? params_.obstacle_bodies_file.c_str() : params_.obstacle_mask_file.c_str(),
                        params_.mask_frontal_height, solid, grid_.plan());
            for (int b = 0; b < params_.body_count(); ++b)
                std::printf("  Body %d: %d cells, D=%d\n", b + 1, params_.body_cells[(size_t)b], params_.body_height[(size_t)b]);
            std::fflush(stdout);
        } else if (!opt_.quiet) {
            std::printf("  Cylinder: center=(%d,%d), radius=%d cells\n  Solid cells: %d\n  Plan: %s\n",
                        params_.get_cylinder_x(), params_.get_cylinder_y(), params_.get_cylinder_radius_cells(), solid,
                        grid_.plan());
            std::fflush(stdout);
        }
    }

    // One loop body of the reference's run() (LBMSolver.h:49-75). Returns false when iteration t is unstable.
    bool step(int t, IOManager& io) {
        if (t != grid_.steps_done()) throw std::runtime_error("Solver::step: iterations must be taken in order");
        if (t % params_.output_frequency == 0) io.record_forces(t, grid_, params_);
        grid_.advance(1, 0);
        if (!report_stability()) return false;
        after_iteration(t, io);
        return true;
    }

    // Solver::run (LBMSolver.h:43-78). Iterations are queued on the GPU in chunks that end at output iterations;
    // forces come from the device-resident log, the stability word is read once per chunk (the reported timestep
    // is the first unstable iteration, as the reference prints at :62).
    bool run(IOManager& io) {
        if (!opt_.quiet) { std::printf("Starting LBM cylinder flow simulation...\n"); std::fflush(stdout); }
        const int T = params_.num_timesteps, of = std::max(1, params_.output_frequency);
        if (params_.bodied()) io.open_body_forces();
        if (params_.probes()) io.open_probes();
        const auto w0 = std::chrono::steady_clock::now();
        int t = grid_.steps_done();
        const int t_begin = t;
        while (t < T) {
            const int snap = ((std::max(t, 1) + of - 1) / of) * of;      // next iteration > 0 with t % of == 0
            const int stop = std::min(T, snap + 1);                       // run through it: the snapshot follows it
            grid_.advance(stop - t, of);
            const int bad = grid_.first_unstable_step();
            for (const auto& r : grid_.drain_force_log())
                if (bad < 0 || r.timestep <= bad) io.append_force_row(r.timestep, r.fx, r.fy, params_);
            for (const auto& r : grid_.drain_body_force_log())
                if (bad < 0 || r.timestep <= bad) io.append_body_force_row(r.timestep, r.body, r.fx, r.fy, params_);
            for (auto& fr : grid_.drain_frames()) {      // the coarsened frames of this chunk: no full-resolution field is fetched for them
                if (bad >= 0 && fr.timestep > bad) continue;
                if (opt_.async_vtk) io.write_frame_async(std::move(fr.planes), params_, fr.timestep);
                else IOManager::write_frame_vtk(fr.planes, params_, fr.timestep);
            }
            for (const auto& s : grid_.drain_probes())      // the probe samples of this chunk
                if (bad < 0 || s.timestep <= bad) io.append_probe_sample(s.timestep, s.vals, params_);
            if (bad >= 0) {
                std::fprintf(stderr, "Simulation unstable at timestep %d\n", bad);
                return false;
            }
            t = stop;
            after_iteration(t - 1, io);
        }
        io.finish_async();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
        if (!opt_.quiet && T > t_begin)
            std::printf("Time loop: %d steps in %.3f s = %.1f MLUPS (incl. output)\n", T - t_begin, sec,
                        1e-6 * params_.nx * params_.ny * double(T - t_begin) / sec);
        return true;
    }

    // Restart support: continue a run from a state written by save_state (same parameters).
    // (with statistics: the sums travel beside the checkpoint as <file>.stats; a restart without that file starts its averages afresh)
    void load_state(const std::string& path) {
        grid_.load_state(path);
        if (params_.stats() && grid_.load_stats(path + ".stats") && !opt_.quiet)
            std::printf("Statistics restored from %s.stats: %d samples\n", path.c_str(), grid_.stats_samples());
    }
    void save_state(const std::string& path) const {
        grid_.save_state(path);
        if (params_.stats()) grid_.save_stats(path + ".stats");
    }

    const Grid& get_grid() const { return grid_; }
    Grid& get_grid() { return grid_; }   // (the reference's Solver reaches its Grid's mutable accessors as a member)
    const SimulationParams& get_params() const { return params_; }

private:
    bool report_stability() {
        const int bad = grid_.first_unstable_step();
        if (bad < 0) return true;
        std::fprintf(stderr, "Simulation unstable at timestep %d\n", bad);
        return false;
    }
    // Log line + VTK frame of LBMSolver.h:66-75 for the iteration that has just completed.
    void after_iteration(int t, IOManager& io) {
        if (!(t > 0 && t % params_.output_frequency == 0)) return;
        const double max_vel = grid_.max_velocity();
        if (!opt_.quiet) { std::printf("Timestep %d: max_vel=%.6f\n", t, max_vel); std::fflush(stdout); }
        if (enable_vtk_output_ && t >= params_.vtk_start_step) {
            if (opt_.async_vtk) io.write_vtk_async(grid_.ux_field(), grid_.uy_field(), grid_.rho_field(), params_, t);
            else IOManager::write_vtk_timestep(grid_.ux_field(), grid_.uy_field(), grid_.rho_field(), params_, t);
        }
    }

    SimulationParams params_;
    BackendOptions opt_;
    Grid grid_;
    bool enable_vtk_output_;
};

}  // namespace LBM
