// host/lbm/grid.hpp — LBM::Grid: the surface of the reference's Grid (LBMGrid.h:105-150,285,319) backed by the HIP
// library. The populations live on the GPU(s) (SoA planes, include/lbm_hip.h); the accessors below serve host mirrors
// that are refreshed lazily from the device whenever the device state has advanced.
//
// Decomposition. The reference's Grid is one MPI rank's block of a 2-D Cartesian topology, and Solver / IOManager gather
// across ranks (LBMGrid.h:347-392, LBMSolver.h:269-362, LBMIO.h:167-168,225-300). Here ONE Grid is the whole lattice and
// owns N row strips, one lbm_ctx each, on one or several GPUs of the node (lbm_group_*): the strips advance in lockstep
// with their halo rows exchanged device to device, and the library does the gathers (lbm_group_get_* / lbm_group_drain_*:
// rows stacked by y_start, force partial sums added in strip order, the stability word reduced by min, max|u| by max):
// every accessor below that returns a result of the whole lattice is one such call.
#pragma once
#include "../../../include/lbm_hip.h"
#include "params.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace LBM {

class Grid {
public:
    Grid(const SimulationParams& p, const BackendOptions& opt = {}) : nx_(p.nx), ny_(p.ny) {
        const int ndev = std::max(1, std::min(opt.gpus, lbm_device_count()));
        int nstrips = opt.strips > 0 ? opt.strips : ndev;
        if (nstrips > ny_) nstrips = ny_;
        // Grid::initialise_2d_topology (LBMGrid.h:347-364) as a 1-D split of the rows: the first ny % n strips get one more
        const int base = ny_ / nstrips, rem = ny_ % nstrips;
        int y = 0;
        for (int k = 0; k < nstrips; ++k) {
            const int n = base + (k < rem ? 1 : 0);
            lbm_params lp{};
            lp.tau = p.tau; lp.inlet_velocity = p.inlet_velocity; lp.nx = p.nx; lp.ny = p.ny;
            lp.cylinder_x = p.cylinder_x; lp.cylinder_y = p.cylinder_y; lp.cylinder_radius = p.cylinder_radius;
            lp.y_start = y; lp.local_ny = n;
            lp.precision = opt.fp32 ? LBM_PRECISION_F32 : LBM_PRECISION_F64;
            lp.force_log_capacity = 0;
            lbm_ctx* c = nullptr;
            const int dev = (opt.device + k % ndev) % std::max(1, lbm_device_count());
            check(lbm_create(&lp, dev, &c), "lbm_create");
            ctx_.push_back(c);
            y0_.push_back(y);
            nyl_.push_back(n);
            devs_.push_back(dev);
            check(lbm_set_option(c, "tune", opt.tune ? 1 : 0), "lbm_set_option");
            check(lbm_set_option(c, "arith", opt.contracted ? 1 : 0), "lbm_set_option");
            if (p.bodied()) check(lbm_set_body_labels(c, p.obstacle_mask.data(), p.nx, p.ny), "lbm_set_body_labels");
            else if (p.masked()) check(lbm_set_solid_mask(c, p.obstacle_mask.data(), p.nx, p.ny), "lbm_set_solid_mask");
            if (p.profiled()) check(lbm_set_inlet_profile(c, p.inlet_profile.data(), p.ny), "lbm_set_inlet_profile");
            if (p.scheduled())   // every strip is given the same schedule: the halo rows a strip recomputes use the same global iteration
                check(lbm_set_inlet_schedule(c, p.inlet_schedule.data(), (int)p.inlet_schedule.size(), p.inlet_schedule_mode), "lbm_set_inlet_schedule");
            if (p.les()) check(lbm_set_smagorinsky(c, p.smagorinsky_cs), "lbm_set_smagorinsky");
            if (p.trt()) check(lbm_set_trt(c, p.trt_magic), "lbm_set_trt");
            if (p.forced()) check(lbm_set_forcing(c, p.forcing_x, p.forcing_y), "lbm_set_forcing");   // (every strip the same force)
            if (p.mrt()) check(lbm_set_mrt(c, p.mrt_bulk_rate, p.mrt_magic), "lbm_set_mrt");
            if (p.sponge()) check(lbm_set_sponge(c, p.sponge_width, p.sponge_tau_end), "lbm_set_sponge");   // (every strip the same pair: strips cut rows)
            if (p.walled())      // every strip carries both walls; only the strips that hold row 0 / ny - 1 use them
                for (int side = 0; side < 2; ++side) check(lbm_set_wall(c, side, p.wall_kind[side], p.wall_velocity[side]), "lbm_set_wall");
            if (p.ported())      // every strip carries both ports
                for (int side = 0; side < 2; ++side) check(lbm_set_port(c, side, p.port_kind[side], p.port_value[side]), "lbm_set_port");
            if (p.periodic_y) check(lbm_set_periodic_y(c, 1), "lbm_set_periodic_y");   // (every strip: the group joins strip n-1 to strip 0)
            y += n;
        }
        check(lbm_group_link(group(), num_strips(), opt.rccl ? 1 : 0), "lbm_group_link");
        if (!opt.quiet) {   // the banner of Grid::Grid (LBMGrid.h:92-102), restated for this backend
            std::printf("MI355X HIP Grid\n  Global domain: %dx%d\n  GPUs: %d, row strips: %d (halo transport: %s)\n"
                        "  Local with ghosts: %dx%d\n  Ghost layers: 1\n  Precision: %s, collision arithmetic: %s\n"
                        "  Memory on device: %.2f MB\n",
                        nx_, ny_, ndev, nstrips, nstrips == 1 ? "none" : (opt.rccl ? "RCCL send/recv" : "peer copies"),
                        nx_ + 2, ny_ + 2, opt.fp32 ? "fp32" : "fp64", opt.contracted ? "FMA-contracted" : "strict IEEE",
                        2.0 * 9.0 * (nx_ + 2.0) * (ny_ + 2.0) * (opt.fp32 ? 4 : 8) / (1024.0 * 1024.0));
        }
    }
    ~Grid() {
        for (lbm_ctx* c : ctx_) lbm_destroy(c);
    }
    Grid(const Grid&) = delete;
    Grid& operator=(const Grid&) = delete;

    // ---- geometry / sizes (LBMGrid.h:129-150): this Grid is the whole lattice ----
    int x_start() const { return 0; }
    int y_start() const { return 0; }
    int local_nx() const { return nx_; }
    int local_ny() const { return ny_; }
    int total_nx() const { return nx_ + 2; }
    int total_ny() const { return ny_ + 2; }
    int global_nx() const { return nx_; }
    int global_ny() const { return ny_; }
    int mpi_rank() const { return 0; }
    int mpi_size() const { return 1; }
    bool is_left_boundary() const { return true; }
    bool is_right_boundary() const { return true; }
    bool is_bottom_boundary() const { return true; }
    bool is_top_boundary() const { return true; }
    bool is_solid(int x, int y) const { ensure_solid(); return solid_[idx(x, y)] != 0; }
    // the strips behind it
    int num_strips() const { return (int)ctx_.size(); }
    int strip_y_start(int k) const { return y0_[(size_t)k]; }
    int strip_rows(int k) const { return nyl_[(size_t)k]; }
    int strip_device(int k) const { return devs_[(size_t)k]; }

    // ---- macroscopic fields, interior coordinates (LBMGrid.h:124-129). The non-const forms hand out the host mirror,
    // as the reference hands out its arrays: values written there are overwritten by the next iteration's collision. ----
    const double& rho(int x, int y) const { ensure_macros(); return rho_[idx(x, y)]; }
    const double& ux(int x, int y) const { ensure_macros(); return ux_[idx(x, y)]; }
    const double& uy(int x, int y) const { ensure_macros(); return uy_[idx(x, y)]; }
    double& rho(int x, int y) { ensure_macros(); return rho_[idx(x, y)]; }
    double& ux(int x, int y) { ensure_macros(); return ux_[idx(x, y)]; }
    double& uy(int x, int y) { ensure_macros(); return uy_[idx(x, y)]; }
    const std::vector<double>& rho_field() const { ensure_macros(); return rho_; }
    const std::vector<double>& ux_field() const { ensure_macros(); return ux_; }
    const std::vector<double>& uy_field() const { ensure_macros(); return uy_; }

    // ---- populations, ghost-inclusive coordinates (LBMGrid.h:113-122). f_current is the state the next iteration's
    // collision reads: values written through the non-const forms are uploaded before the next iteration (interior
    // cells; ghost cells are owned by the halo logic). f_next is dead between iterations in the reference (collision
    // overwrites it), so writes to it stay in the host mirror. ----
    const double& f_current(int gx, int gy, int i) const { ensure_f(0); return fc_[fidx(gx, gy, i)]; }
    const double& f_next(int gx, int gy, int i) const { ensure_f(1); return fn_[fidx(gx, gy, i)]; }
    double& f_current(int gx, int gy, int i) { ensure_f(0); fc_dirty_ = true; return fc_[fidx(gx, gy, i)]; }
    double& f_next(int gx, int gy, int i) { ensure_f(1); return fn_[fidx(gx, gy, i)]; }
    double* f_current_ptr(int gx, int gy) { ensure_f(0); fc_dirty_ = true; return &fc_[fidx(gx, gy, 0)]; }
    double* f_next_ptr(int gx, int gy) { ensure_f(1); return &fn_[fidx(gx, gy, 0)]; }

    // Grid::check_stability (LBMGrid.h:285-317): evaluated on the device inside every step kernel; min over the strips
    // (the reference's MPI_Allreduce(MIN) of the flag, :315).
    bool check_stability() const { return first_unstable_step() < 0; }
    int first_unstable_step() const {
        int first = -1;
        check(lbm_group_first_unstable_step(group(), num_strips(), &first), "lbm_group_first_unstable_step");
        return first;
    }
    // Grid::max_velocity (LBMGrid.h:319-344): max over the strips, then the square root
    double max_velocity() const {
        double m = 0.0;
        check(lbm_group_max_velocity_sq(group(), num_strips(), &m), "lbm_group_max_velocity_sq");
        return std::sqrt(m);
    }

    // ---- device control used by Solver / IOManager ----
    int setup_and_initialise() {   // setup_geometry + initialise (LBMGrid.h:152-246) + collision of iteration 0
        int solid = 0;
        check(lbm_group_initialise(group(), num_strips(), &solid), "lbm_group_initialise");
        invalidate();
        return solid;
    }
    void advance(int nsteps, int output_frequency) {
        upload_f_current();
        check(lbm_group_step(group(), num_strips(), nsteps, output_frequency), "lbm_group_step");
        invalidate();
    }
    int steps_done() const { return lbm_steps_done(ctx_[0]); }
    // IOManager::record_forces' MPI_Reduce(SUM) over the ranks (LBMIO.h:167-168): each strip sums the links whose fluid
    // end it owns
    void forces_now(double& fx, double& fy) const { check(lbm_group_get_forces(group(), num_strips(), &fx, &fy), "lbm_group_get_forces"); }
    std::vector<lbm_force_row> drain_force_log() const {
        std::vector<lbm_force_row> rows(4096);
        const int got = lbm_group_drain_force_log(group(), num_strips(), rows.data(), (int)rows.size());
        check(got, "lbm_group_drain_force_log");
        rows.resize((size_t)got);
        return rows;
    }
    // per-body forces (lbm_set_body_labels; the reference has none): the strips' partial sums added per (sample, body) in strip order
    int body_count() const { return lbm_body_count(ctx_[0]); }
    std::vector<lbm_body_force_row> body_forces_now(int timestep) const {
        const int B = body_count();
        std::vector<lbm_body_force_row> sum((size_t)B);
        std::vector<double> fxy(2 * (size_t)B);
        if (B > 0) check(lbm_group_get_body_forces(group(), num_strips(), fxy.data()), "lbm_group_get_body_forces");
        for (int b = 0; b < B; ++b) sum[(size_t)b] = {timestep, b + 1, fxy[2 * (size_t)b], fxy[2 * (size_t)b + 1]};
        return sum;
    }
    std::vector<lbm_body_force_row> drain_body_force_log() const {
        std::vector<lbm_body_force_row> rows((size_t)body_count() * 4096);
        const int got = lbm_group_drain_body_force_log(group(), num_strips(), rows.data(), (int)rows.size());
        check(got, "lbm_group_drain_body_force_log");
        rows.resize((size_t)got);
        return rows;
    }
    // checkpoint / restart (build-only feature; the reference keeps its state in memory only): one file per strip
    // (`path` itself for a single strip, `path.k` otherwise)
    void save_state(const std::string& path) const {
        for (size_t k = 0; k < ctx_.size(); ++k) check(lbm_save_state(ctx_[k], strip_file(path, k).c_str()), "lbm_save_state");
    }
    void load_state(const std::string& path) {
        for (size_t k = 0; k < ctx_.size(); ++k) check(lbm_load_state(ctx_[k], strip_file(path, k).c_str()), "lbm_load_state");
        check(lbm_group_refresh_halos(group(), num_strips()), "lbm_group_refresh_halos");
        invalidate();
    }
    // time-averaged statistics (lbm_stats_*; the reference has none): begun on every strip, the six sums gathered like the macroscopic
    // fields (rows concatenated by y_start) into [6][ny][nx]; the sample count is the same on every strip
    void stats_begin(int from_step) {
        for (lbm_ctx* c : ctx_) check(lbm_stats_begin(c, from_step), "lbm_stats_begin");
    }
    int stats_samples() const {
        const int samples = lbm_group_stats_samples(group(), num_strips());
        check(samples, "lbm_group_stats_samples");
        return samples;
    }
    std::vector<double> stat_sums() const {
        std::vector<double> all(6 * static_cast<size_t>(nx_) * ny_);
        check(lbm_group_get_stat_sums(group(), num_strips(), all.data()), "lbm_group_get_stat_sums");
        return all;
    }
    void stats_restore(const std::vector<double>& all, int samples) {
        if (all.size() != 6 * static_cast<size_t>(nx_) * ny_) throw std::runtime_error("statistics of a different lattice");
        check(lbm_group_stats_restore(group(), num_strips(), all.data(), samples), "lbm_group_stats_restore");
    }
    // the sums beside a checkpoint (checkpoints do not carry them): "LBMSTAT1", nx, ny, samples, then [6][ny][nx] doubles of the
    // whole lattice, whatever the strips. load_stats: false when the file does not exist (the averages start afresh).
    void save_stats(const std::string& path) const {
        const std::vector<double> all = stat_sums();
        const int head[3] = {nx_, ny_, stats_samples()};
        std::FILE* fp = std::fopen(path.c_str(), "wb");
        const bool ok = fp && std::fwrite("LBMSTAT1", 1, 8, fp) == 8 && std::fwrite(head, sizeof(int), 3, fp) == 3 &&
                        std::fwrite(all.data(), sizeof(double), all.size(), fp) == all.size();
        if (fp) std::fclose(fp);
        if (!ok) throw std::runtime_error("cannot write " + path);
    }
    bool load_stats(const std::string& path) {
        std::FILE* fp = std::fopen(path.c_str(), "rb");
        if (!fp) return false;
        char magic[8];
        int head[3] = {0, 0, 0};
        std::vector<double> all(6 * static_cast<size_t>(nx_) * ny_);
        const bool ok = std::fread(magic, 1, 8, fp) == 8 && std::memcmp(magic, "LBMSTAT1", 8) == 0 && std::fread(head, sizeof(int), 3, fp) == 3 &&
                        head[0] == nx_ && head[1] == ny_ && head[2] >= 0 && std::fread(all.data(), sizeof(double), all.size(), fp) == all.size();
        std::fclose(fp);
        if (!ok) throw std::runtime_error(path + " does not hold the statistics of this lattice");
        stats_restore(all, head[2]);
        return true;
    }
    // coarsened flow frames (lbm_frames_*; the reference has none): begun on every strip; a drained frame is the strips' rows
    // concatenated by y_start into [4][ny / k][nx / k] (rho, ux, uy, vorticity). Every strip samples at the same iterations.
    struct CoarseFrame { int timestep; std::vector<float> planes; };
    void frames_begin(int k, int capacity) {
        for (lbm_ctx* c : ctx_) check(lbm_frames_begin(c, k, capacity), "lbm_frames_begin");
        frame_k_ = k;
    }
    std::vector<CoarseFrame> drain_frames() const {
        std::vector<CoarseFrame> out;
        if (frame_k_ < 1) return out;
        const int m = lbm_group_frames_pending(group(), num_strips());
        check(m, "lbm_group_frames_pending");
        const size_t per = 4 * static_cast<size_t>(nx_ / frame_k_) * static_cast<size_t>(ny_ / frame_k_);
        std::vector<float> all((size_t)m * per);
        std::vector<int> ts((size_t)m);
        check(lbm_group_drain_frames(group(), num_strips(), ts.data(), all.data(), m), "lbm_group_drain_frames");
        for (int j = 0; j < m; ++j) out.push_back({ts[(size_t)j], {all.begin() + (size_t)j * per, all.begin() + ((size_t)j + 1) * per}});
        return out;
    }
    // point probes (lbm_probes_*; the reference has none): every strip is given the same global points and samples those of its rows
    // (+0.0 for the others); a drained sample is the strips' values added up in strip order, like the partial force sums.
    struct ProbeSample { int timestep; std::vector<double> vals; };      // [n][3]: rho, ux, uy
    void probes_begin(const std::vector<double>& xy, int capacity) {
        for (lbm_ctx* c : ctx_) check(lbm_probes_begin(c, xy.data(), (int)(xy.size() / 2), capacity), "lbm_probes_begin");
    }
    std::vector<ProbeSample> drain_probes() const {
        std::vector<ProbeSample> out;
        const int m = lbm_group_probes_pending(group(), num_strips());
        check(m, "lbm_group_probes_pending");
        const size_t per = 3 * (size_t)lbm_probes_count(ctx_[0]);
        std::vector<double> all((size_t)m * per);
        std::vector<int> ts((size_t)m);
        check(lbm_group_drain_probes(group(), num_strips(), ts.data(), all.data(), m), "lbm_group_drain_probes");
        for (int j = 0; j < m; ++j) out.push_back({ts[(size_t)j], {all.begin() + (size_t)j * per, all.begin() + ((size_t)j + 1) * per}});
        return out;
    }
    const char* plan() const { return lbm_plan(ctx_[0]); }
    lbm_ctx* handle(int k = 0) const { return ctx_[(size_t)k]; }

private:
    lbm_ctx** group() const { return const_cast<lbm_ctx**>(ctx_.data()); }      // the group as linked, for the lbm_group_* calls
    static void check(int rc, const char* what) {
        if (rc < 0) throw std::runtime_error(std::string(what) + ": " + lbm_last_error());
    }
    std::string strip_file(const std::string& path, size_t k) const {
        return ctx_.size() == 1 ? path : path + "." + std::to_string(k);
    }
    size_t idx(int x, int y) const { return static_cast<size_t>(y) * nx_ + x; }
    size_t fidx(int gx, int gy, int i) const { return (static_cast<size_t>(gy) * (nx_ + 2) + gx) * Q + i; }
    void invalidate() { macros_ok_ = false; f_ok_[0] = f_ok_[1] = false; fc_dirty_ = false; }
    void ensure_macros() const {   // the gather of Solver::write_vtk_frame (LBMSolver.h:340-357): strips stacked by y_start
        if (macros_ok_) return;
        const size_t cells = static_cast<size_t>(nx_) * ny_;
        rho_.resize(cells); ux_.resize(cells); uy_.resize(cells);
        check(lbm_group_get_macros(group(), num_strips(), rho_.data(), ux_.data(), uy_.data()), "lbm_group_get_macros");
        macros_ok_ = true;
    }
    void ensure_f(int which) const {
        if (f_ok_[which]) return;
        auto& v = which == 0 ? fc_ : fn_;
        v.resize(static_cast<size_t>(nx_ + 2) * Q * (ny_ + 2));
        check(lbm_group_get_populations(group(), num_strips(), which, v.data()), "lbm_group_get_populations");
        f_ok_[which] = true;
    }
    void upload_f_current() {   // values a client wrote through f_current(x,y,i): re-collided into the device state
        if (!fc_dirty_) return;
        const size_t row = static_cast<size_t>(nx_ + 2) * Q;
        for (size_t k = 0; k < ctx_.size(); ++k)
            check(lbm_set_f_current(ctx_[k], fc_.data() + static_cast<size_t>(y0_[k]) * row), "lbm_set_f_current");
        check(lbm_group_refresh_halos(group(), num_strips()), "lbm_group_refresh_halos");
        fc_dirty_ = false;
    }
    void ensure_solid() const {
        if (!solid_.empty()) return;
        solid_.resize(static_cast<size_t>(nx_) * ny_);
        for (size_t k = 0; k < ctx_.size(); ++k)
            check(lbm_get_solid(ctx_[k], solid_.data() + static_cast<size_t>(y0_[k]) * nx_), "lbm_get_solid");
    }

    int nx_, ny_;
    std::vector<lbm_ctx*> ctx_;
    std::vector<int> y0_, nyl_, devs_;
    mutable std::vector<double> rho_, ux_, uy_, fc_, fn_;
    mutable std::vector<unsigned char> solid_;
    mutable bool macros_ok_ = false;
    mutable bool f_ok_[2] = {false, false};
    bool fc_dirty_ = false;
    int frame_k_ = 0;
};

}  // namespace LBM
