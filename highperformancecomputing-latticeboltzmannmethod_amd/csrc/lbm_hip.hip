// csrc/lbm_hip.hip — host side of liblbm_hip.so: the C-ABI of include/lbm_hip.h over the gfx950 kernels in
// lbm_kernels.hpp. Plain HIP runtime + RCCL; no torch types, no CPU fallback.
#include "lbm_kernels.hpp"
#include "lbm_col_api.hpp"
#include "lbm_launch_k.hpp"
#include "lbm_frames.hpp"
#include "lbm_probes.hpp"
#include "lbm_plan.hpp"
#include "lbm_gather.hpp"
#include "lbm_geom.hpp"
#include "lbm_ckpt.hpp"
#include "../../include/lbm_hip.h"

#include <rccl/rccl.h>

#include <climits>
#include <cstdint>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

using namespace lbmk;

#include "lbm_ctx.hpp"

namespace {
#include "lbm_launch.inc.hpp"
#include "lbm_strips.inc.hpp"
#include "lbm_tune.inc.hpp"
#include "lbm_steps.inc.hpp"
#include "lbm_choreo.inc.hpp"
}  // namespace

namespace {
int allreduce_doubles(lbm_ctx* c, double* vals, int n, int op) {
    HIPCHK(hipMemcpyAsync(c->d_red, vals, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const ncclRedOp_t rop = op == 0 ? ncclSum : (op == 1 ? ncclMax : ncclMin);
    NCCLCHK(ncclAllReduce(c->d_red, c->d_red, n, ncclDouble, rop, c->comm, c->stream));
    HIPCHK(hipMemcpyAsync(vals, c->d_red, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LBM_OK;
}
}  // namespace

namespace {
// f_eq(rho=1, u=(ux,0)) as Grid::initialise evaluates it (LBMUtils.h:9-12,22-65): the initial state of the inflow, uniform
// (inlet_velocity) or per row (lbm_set_inlet_profile)
void feq_inflow(double ux, double (&f)[Q]) {
    const double uy = 0.0, rho = 1.0;
    const double usq = ux * ux + uy * uy, t3 = 1.5 * usq;
    f[0] = wgt<double>(0) * rho * (1.0 - 1.5 * usq);
    for (int i = 1; i < Q; ++i) {
        const double cu = (double)cx(i) * ux + (double)cy(i) * uy;
        f[i] = (wgt<double>(i) * rho) * (((1.0 + 3.0 * cu) - t3) + 4.5 * (cu * cu));
    }
}
// host doubles -> a device table in the context's element type (fp32: converted as inlet_velocity is)
int upload_rows(const lbm_ctx* c, void* dst, const double* v, size_t n) {
    if (c->esize == 4) {
        std::vector<float> w(v, v + n);
        HIPCHK(hipMemcpy(dst, w.data(), n * sizeof(float), hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(dst, v, n * sizeof(double), hipMemcpyHostToDevice));
    }
    return LBM_OK;
}
// The initial equilibria f_eq(1, (u[y], 0)) of every global row into d_feqrow (k_init), replacing an earlier table.
// The tables cover every global row, not only the strip's rows +- GR: the register kernel's garbage cells beyond a partial band
// may evaluate the inlet of any row of the domain, and a whole table keeps that read in bounds without a test in the kernel.
int upload_feqrow(lbm_ctx* c, const double* u, int ny) {
    std::vector<double> feqrow((size_t)ny * Q);
    for (int y = 0; y < ny; ++y) {
        double f[Q];
        feq_inflow(u[y], f);
        for (int i = 0; i < Q; ++i) feqrow[(size_t)y * Q + i] = f[i];
    }
    if (c->d_feqrow) { HIPCHK(hipFree(c->d_feqrow)); c->d_feqrow = nullptr; }
    HIPCHK(hipMalloc(&c->d_feqrow, feqrow.size() * c->esize));
    return upload_rows(c, c->d_feqrow, feqrow.data(), feqrow.size());
}

// v[0 .. ny) by global row -> the table the kernels index by the rows they count: v itself, or — periodic y — rows_glob entries,
// entry r = v[(r - PERIODIC_PAD) mod ny]
std::vector<double> table_rows(const lbm_ctx* c, const double* v) {
    const int ny = c->p.ny, n = rows_glob(c), off = row_offset(c);
    std::vector<double> t((size_t)n);
    for (int r = 0; r < n; ++r) t[(size_t)r] = v[(size_t)(((r - off) % ny + ny) % ny)];
    return t;
}

// ---- the inlet schedule (lbm_set_inlet_schedule) ----
// the argument checks shared by lbm_set_inlet_schedule and lbm_debug_inlet_scale; the text names the offender
int check_schedule(const char* who, const double* s, int n, int mode) {
    if (n < 0 || n > LBM_INLET_SCHEDULE_MAX) return fail(LBM_ERR_ARG, "%s: n = %d (0 .. %d only)", who, n, LBM_INLET_SCHEDULE_MAX);
    if (n > 0 && !s) return fail(LBM_ERR_ARG, "%s: null table with n = %d", who, n);
    if (mode != LBM_INLET_HOLD && mode != LBM_INLET_REPEAT) return fail(LBM_ERR_ARG, "%s: mode = %d (0 hold or 1 repeat only)", who, mode);
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(s[k])) return fail(LBM_ERR_ARG, "%s: entry %d is %g (finite factors only)", who, k, s[k]);
    return LBM_OK;
}
// the device block the kernels read: {n, mode}, then the factors in the element type (lbm_kernels.hpp inlet_sched_at)
template <typename T>
int upload_schedule(lbm_ctx* c) {
    const size_t n = c->sched.size(), bytes = INLET_SCHED_HEAD * sizeof(int) + n * sizeof(T);
    std::vector<unsigned char> h(bytes);
    const int head[INLET_SCHED_HEAD] = {(int)n, c->sched_mode};
    memcpy(h.data(), head, sizeof(head));
    T* tab = reinterpret_cast<T*>(h.data() + sizeof(head));
    for (size_t k = 0; k < n; ++k) tab[k] = (T)c->sched[k];
    HIPCHK(hipMalloc(&c->d_sched, bytes));
    HIPCHK(hipMemcpy(c->d_sched, h.data(), bytes, hipMemcpyHostToDevice));
    return LBM_OK;
}
// lbm_initialise with a schedule set, where profile and schedule are both known: the inlet divides by 1 - u[y] * s[k]; the initial state
// is that of the profile u0[y] = u[y] * s[0], formed here in double (d_feqrow for k_init, d_urow0 for the initial snapshot).
int prepare_schedule(lbm_ctx* c) {
    const int ny = c->p.ny;
    double smax = c->sched[0], smin = c->sched[0];
    for (double v : c->sched) { smax = std::max(smax, v); smin = std::min(smin, v); }
    for (int y = 0; y < ny; ++y) {
        const double u = c->h_urow[(size_t)y];
        if (u * smax < 1.0 && u * smin < 1.0) continue;
        for (size_t k = 0; k < c->sched.size(); ++k)
            if (!(u * c->sched[k] < 1.0))
                return fail(LBM_ERR_ARG, "lbm_initialise: inlet row %d (velocity %g) times schedule entry %d (factor %g) is %g (products below 1 only)",
                            y, u, (int)k, c->sched[k], u * c->sched[k]);
    }
    std::vector<double> u0((size_t)ny);
    for (int y = 0; y < ny; ++y) u0[(size_t)y] = c->h_urow[(size_t)y] * c->sched[0];
    const std::vector<double> t0 = table_rows(c, u0.data());
    if (int rc = upload_feqrow(c, t0.data(), (int)t0.size())) return rc;
    if (c->d_urow0) { HIPCHK(hipFree(c->d_urow0)); c->d_urow0 = nullptr; }
    HIPCHK(hipMalloc(&c->d_urow0, t0.size() * c->esize));
    return upload_rows(c, c->d_urow0, t0.data(), t0.size());
}

// ---- periodic y (lbm_set_periodic_y): what lbm_initialise builds for the rows the kernels count (lbm_launch.inc.hpp row_offset) ----
// The refusals only lbm_initialise can make, each naming the offender.
int refuse_periodic(const lbm_ctx* c) {
    if (c->has_walls())
        return fail(LBM_ERR_ARG, "lbm_initialise: a %s south wall and a %s north wall (lbm_set_wall) beside periodic y (lbm_set_periodic_y): no wall rule runs on a periodic lattice",
                    wall_kind_name(c->wall_kind[0]), wall_kind_name(c->wall_kind[1]));
    if (c->body_n > 0 && (c->hmask.by0 == 0 || c->hmask.by1 == c->p.ny - 1))
        return fail(LBM_ERR_ARG, "lbm_initialise: body labels (lbm_set_body_labels) with a labelled cell on row %d beside periodic y: a body's box is clipped at the domain, "
                                 "its links across the seam would be missed", c->hmask.by0 == 0 ? 0 : c->p.ny - 1);
    if (c->comm && c->nranks > 1 && c->group_n <= 1)
        return fail(LBM_ERR_ARG, "lbm_initialise: a communicator of %d ranks (lbm_comm_init) beside periodic y: rings of processes are not built", c->nranks);
    if (c->layout_pinned && c->layout == 0) return fail(LBM_ERR_ARG, "lbm_initialise: option layout = 0 (planar) beside periodic y: a periodic context is a strip, row-interleaved only");
    if (c->split_pinned && c->split) return fail(LBM_ERR_ARG, "lbm_initialise: option split = %d beside periodic y: row-range launches exist for a whole domain only", c->split);
    if (c->loopback) return fail(LBM_ERR_ARG, "lbm_initialise: option loopback = %d (a test transport, with walls) beside periodic y", c->loopback);
    if (c->nyl < 2 * HR1) return fail(LBM_ERR_ARG, "lbm_initialise: a strip of %d rows beside periodic y: a strip with neighbours needs at least %d rows", c->nyl, 2 * HR1);
    return LBM_OK;
}
// The device copies of a packed mask's bitmap and coarse table (owned by the context from the moment they exist: lbm_destroy frees them)
// in place of the ones it had, and the partial sums of the force kernel's chunks: what lbm_set_solid_mask and prepare_periodic upload.
int upload_mask(lbm_ctx* c, const HostMask& h) {
    if (c->mview.bits) { HIPCHK(hipFree((void*)c->mview.bits)); c->mview.bits = nullptr; }
    if (c->mview.sat) { HIPCHK(hipFree((void*)c->mview.sat)); c->mview.sat = nullptr; }
    if (c->d_fpart) { HIPCHK(hipFree(c->d_fpart)); c->d_fpart = nullptr; }
    c->mview = h.view();
    c->mview.bits = nullptr; c->mview.sat = nullptr;
    unsigned long long* dbits = nullptr;
    int* dsat = nullptr;
    HIPCHK(hipMalloc(&dbits, std::max<size_t>(1, h.bits.size()) * sizeof(unsigned long long)));
    c->mview.bits = dbits;
    HIPCHK(hipMalloc(&dsat, h.sat.size() * sizeof(int)));
    c->mview.sat = dsat;
    HIPCHK(hipMemcpy(dbits, h.bits.data(), h.bits.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsat, h.sat.data(), h.sat.size() * sizeof(int), hipMemcpyHostToDevice));
    c->fpart_chunks = (int)(((long)c->nx * c->nyl + FORCE_CHUNK - 1) / FORCE_CHUNK);
    HIPCHK(hipMalloc(&c->d_fpart, 2 * sizeof(double) * (size_t)std::max(1, c->fpart_chunks)));
    return LBM_OK;
}
// The row tables with PERIODIC_PAD wrapped rows each side, and the wrapped window of the geometry — the user's mask, or the disc
// rasterised by the disc test, so that its image across the seam exists — in place of what the setters uploaded.
int prepare_periodic(lbm_ctx* c) {
    const std::vector<double> t = table_rows(c, c->h_urow.data());
    if (c->d_urow) { HIPCHK(hipFree(c->d_urow)); c->d_urow = nullptr; }
    HIPCHK(hipMalloc(&c->d_urow, t.size() * c->esize));
    if (int rc = upload_rows(c, c->d_urow, t.data(), t.size())) return rc;
    if (c->has_profile && !c->has_sched()) { if (int rc = upload_feqrow(c, t.data(), (int)t.size())) return rc; }
    const int nx = c->nx, ny = c->p.ny;
    const double r2 = (double)(c->cyl_r * c->cyl_r);
    auto solid = [&](int x, int w, int y) {
        if (c->has_mask) return c->user_mask[(size_t)w * nx + x] != 0;
        const double dx = x - c->cyl_x, dy = y - c->cyl_y;      // (the test of lbm_get_solid and is_solid_cell)
        return dx * dx + dy * dy <= r2;
    };
    HostMask h = pack_mask_periodic(solid, nx, ny, c->p.y_start, c->nyl, PERIODIC_PAD);
    if (int rc = upload_mask(c, h)) return rc;
    c->pmask = std::move(h);
    return LBM_OK;
}
}  // namespace

// ---- checkpoint / restart: the format, the table of its optional fields and the refusals are lbm_ckpt.hpp ----
namespace {
// what a checkpoint of this context says in its head, and what the head of a file it loads must say
lbm_ckpt_head ckpt_head_of(const lbm_ctx* c) {
    lbm_ckpt_head h{};
    h.nx = c->nx; h.ny = c->p.ny; h.y_start = c->p.y_start; h.local_ny = c->nyl; h.precision = c->p.precision;
    h.steps_done = c->steps_done; h.tau = c->p.tau; h.inlet_velocity = c->p.inlet_velocity;
    h.cylinder_x = c->p.cylinder_x; h.cylinder_y = c->p.cylinder_y; h.cylinder_radius = c->p.cylinder_radius;
    h.has_mask = c->has_mask; h.mask_digest = c->hmask.digest;
    h.has_profile = c->has_profile; h.profile_digest = c->prof_digest;
    h.collision = c->collision; h.collision_param[0] = c->collision_param; h.collision_param[1] = c->collision_param2;
    h.has_walls = c->has_walls();
    h.walls[0] = (double)c->wall_kind[0]; h.walls[1] = c->wall_u[0]; h.walls[2] = (double)c->wall_kind[1]; h.walls[3] = c->wall_u[1];
    h.has_sched = c->has_sched(); h.sched_digest = c->sched_digest;
    h.has_ports = c->has_ports();
    h.ports[0] = (double)c->port_kind[0]; h.ports[1] = c->port_value[0]; h.ports[2] = (double)c->port_kind[1]; h.ports[3] = c->port_value[1];
    h.has_periodic_y = c->periodic_y;
    return h;
}
// lbm_load_state and lbm_debug_ckpt_load: the head in the first n bytes of `path` against the loading context's: the bytes it takes and
// what it says, or the refusal
int accept_head(const char* path, const unsigned char* bytes, int n, const lbm_ckpt_head& here, lbm_ckpt_head* file) {
    const int used = ckpt_parse(bytes, n, file);
    if (!used) return fail(LBM_ERR_ARG, "%s is not a checkpoint", path);
    const std::string why = ckpt_refusal(*file, here);
    if (!why.empty()) return fail(LBM_ERR_ARG, "checkpoint %s was written %s", path, why.c_str());
    return used;
}

// The populations of a checkpoint, the interior rows of buf[cur] as [9][local_ny][nx]: written to fp, or (load) read from it. buf[cur]
// comes down whole first: on a load it already holds P_0 with all ghost / solid constants in place and only its interior is overwritten
// (the previous-iteration buffer's ghost frame is not needed: it is only read by snapshots after the next step).
template <typename T>
int transfer_interior(lbm_ctx* c, FILE* fp, bool load) {
    std::vector<T> host(c->total);
    HIPCHK(hipMemcpyAsync(host.data(), c->buf[c->cur], c->total * c->esize, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t nx = (size_t)c->nx;
    for (int i = 0; i < Q; ++i)
        for (int y = 0; y < c->nyl; ++y) {
            T* row = host.data() + (size_t)i * c->plane + (size_t)(y + GR) * c->pitch + c->xoff;
            if ((load ? fread(row, sizeof(T), nx, fp) : fwrite(row, sizeof(T), nx, fp)) != nx) return fail(LBM_ERR_ARG, load ? "short read" : "short write");
        }
    if (!load) return LBM_OK;
    HIPCHK(hipMemcpyAsync(c->buf[c->cur], host.data(), c->total * c->esize, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LBM_OK;
}

// What the two force-log drains share: up to `m` of the oldest samples of a log of B rows (t, fx, fy) per sample leave the ring and are
// unpacked into the caller's rows through `put(row, k, t)`, k counting the rows drained; the samples drained, or an error.
template <typename Row, typename Put>
int drain_force_rows(lbm_ctx* c, DeviceRing<double>& log, int B, Row* rows, int m, Put put) {
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> h(3 * (size_t)B * std::max(1, std::min(m, log.ix.count)));
    const int n = log.drain(c->stream, h.data(), nullptr, m);
    for (size_t k = 0; n > 0 && k < (size_t)B * n; ++k) {
        put(rows[k], k, (int)h[3 * k]);
        rows[k].fx = h[3 * k + 1];
        rows[k].fy = h[3 * k + 2];
    }
    return n;
}
}  // namespace

// ---- the two walls (lbm_set_wall) ----
namespace {
// the argument checks shared by lbm_set_wall and lbm_debug_wall_rule; the text names the offender
int check_wall(const char* who, int side, int kind, double velocity) {
    if (side != LBM_WALL_SOUTH && side != LBM_WALL_NORTH) return fail(LBM_ERR_ARG, "%s: side = %d (0 south or 1 north only)", who, side);
    if (kind < LBM_WALL_NOSLIP || kind > LBM_WALL_MOVING) return fail(LBM_ERR_ARG, "%s: kind = %d (0 no-slip, 1 free-slip or 2 moving only)", who, kind);
    if (!std::isfinite(velocity) || std::fabs(velocity) >= 1.0)
        return fail(LBM_ERR_ARG, "%s: velocity = %g (finite values of magnitude below 1 only)", who, velocity);
    if (kind != LBM_WALL_MOVING && velocity != 0.0)
        return fail(LBM_ERR_ARG, "%s: velocity = %g with a %s wall (only a moving wall takes one)", who, velocity, wall_kind_name(kind));
    return LBM_OK;
}
template <typename T>
void debug_wall_rule(int side, int kind, double velocity, const double* in9, double* out9) {
    T f[Q];
    for (int i = 0; i < Q; ++i) f[i] = (T)in9[i];
    wall_rule<T>(f, side == LBM_WALL_SOUTH, side == LBM_WALL_NORTH, side == LBM_WALL_SOUTH ? wall_pack(kind, 0) : wall_pack(0, kind),
                 wall_ks<T>(kind, velocity, kind, velocity));
    for (int i = 0; i < Q; ++i) out9[i] = (double)f[i];
}
}  // namespace

// ---- the two ports (lbm_set_port) ----
namespace {
// the argument checks shared by lbm_set_port and lbm_debug_port_rule; the text names the offender
int check_port(const char* who, int side, int kind, double value) {
    if (side != LBM_PORT_WEST && side != LBM_PORT_EAST) return fail(LBM_ERR_ARG, "%s: side = %d (0 west or 1 east only)", who, side);
    if (kind != LBM_PORT_VELOCITY && kind != LBM_PORT_PRESSURE) return fail(LBM_ERR_ARG, "%s: kind = %d (0 velocity or 1 pressure only)", who, kind);
    if (!std::isfinite(value)) return fail(LBM_ERR_ARG, "%s: value = %g (finite values only)", who, value);
    if (kind == LBM_PORT_PRESSURE && value <= 0.0) return fail(LBM_ERR_ARG, "%s: pressure = %g (a density above 0 only)", who, value);
    if (kind == LBM_PORT_VELOCITY && side == LBM_PORT_EAST && std::fabs(value) >= 1.0)
        return fail(LBM_ERR_ARG, "%s: east velocity = %g (magnitude below 1 only)", who, value);
    if (kind == LBM_PORT_VELOCITY && side == LBM_PORT_WEST && value != 0.0)
        return fail(LBM_ERR_ARG, "%s: value = %g with a west velocity port (it takes inlet_velocity, the inlet profile and the inlet schedule; 0 only)", who, value);
    return LBM_OK;
}
template <typename T>
void debug_port_rule(int side, int kind, double value, double u_in, const double* in9, double* out9, double* rho_out, double* u_out) {
    T f[Q];
    for (int i = 0; i < Q; ++i) f[i] = (T)in9[i];
    const bool west = side == LBM_PORT_WEST;
    const T u_west = (T)u_in;
    T rho = T(0), u = T(0);
    port_rule<T>(f, west, !west, west ? port_pack(kind, PORT_PRESSURE) : port_pack(PORT_VELOCITY, kind), port_ks<T>(value, west ? PORT_PRESSURE : kind, value),
                 [&]() { return u_west; }, rho, u);
    for (int i = 0; i < Q; ++i) out9[i] = (double)f[i];
    if (rho_out) *rho_out = (double)rho;
    if (u_out) *u_out = (double)u;
}
}  // namespace


extern "C" {

const char* lbm_last_error(void) { return g_err; }

int lbm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lbm_create(const lbm_params* p, int device, lbm_ctx** out) {
    if (!p || !out) return fail(LBM_ERR_ARG, "null argument");
    if (p->nx < 1 || p->ny < 1 || !(p->tau > 0.0)) return fail(LBM_ERR_ARG, "bad nx/ny/tau");
    if (p->precision != LBM_PRECISION_F64 && p->precision != LBM_PRECISION_F32)
        return fail(LBM_ERR_ARG, "bad precision %d", p->precision);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(LBM_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(LBM_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    lbm_ctx* c = new (std::nothrow) lbm_ctx();
    if (!c) return fail(LBM_ERR_ALLOC, "out of host memory");
    c->p = *p;
    if (c->p.local_ny <= 0) c->p.local_ny = p->ny - p->y_start;
    if (c->p.y_start < 0 || c->p.y_start + c->p.local_ny > p->ny || c->p.local_ny < 1) {
        delete c;
        return fail(LBM_ERR_ARG, "strip [%d,%d) outside [0,%d)", p->y_start, p->y_start + p->local_ny, p->ny);
    }
    if (c->p.local_ny > 65535) {   // one grid row (grid.y) per lattice row in the single-iteration kernels
        delete c;
        return fail(LBM_ERR_ARG, "a strip is limited to 65535 rows (got %d): cut the domain into more strips", p->local_ny);
    }
    c->device = device;
    c->nx = p->nx;
    c->nyl = c->p.local_ny;
    c->esize = p->precision == LBM_PRECISION_F32 ? 4 : 8;
    const int per128 = (int)(128 / c->esize);
    c->xoff = per128;                                      // interior x=0 starts a 128-byte line
    c->pitch0 = round_up(c->xoff + c->nx + 1, per128);     // ghost column x=nx fits, rows stay 128-B aligned
    configure_layout(c, 0);
    // LBMConfig.h:61-65: truncation toward zero
    c->cyl_x = (int)(p->cylinder_x * p->nx);
    c->cyl_y = (int)(p->cylinder_y * p->ny);
    c->cyl_r = (int)(p->cylinder_radius * p->ny);
    feq_inflow(p->inlet_velocity, c->feq_in);
    c->log_cap = p->force_log_capacity > 0 ? p->force_log_capacity : 4096;
    auto bail = [&](int code) { lbm_destroy(c); return code; };
#define HIPTRY(expr)                                                                                             \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                    \
            return bail(fail(LBM_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)));  \
    } while (0)
    HIPTRY(hipSetDevice(device));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->num_cus = cus;
    }
    HIPTRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {   // the side stream carries the edge bands + exchange, which sit on the critical path: highest priority
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        HIPTRY(hipStreamCreateWithPriority(&c->comm_stream, hipStreamNonBlocking, hi));
    }
    HIPTRY(hipStreamCreateWithFlags(&c->split_stream, hipStreamNonBlocking));      // the second stream of split launches: default priority
    HIPTRY(hipEventCreateWithFlags(&c->ev_edge, hipEventDisableTiming | hipEventDisableSystemFence));   // device-side ordering only
    HIPTRY(hipEventCreateWithFlags(&c->ev_comm, hipEventDisableTiming | hipEventDisableSystemFence));   // device-side ordering only
    HIPTRY(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming | hipEventDisableSystemFence));   // device-side ordering only
    HIPTRY(hipEventCreate(&c->ev_t0));
    HIPTRY(hipEventCreate(&c->ev_t1));
    // the population buffers are allocated by lbm_initialise (the plan decides their layout)
    HIPTRY(hipMalloc(&c->d_unstable, sizeof(int)));
    HIPTRY(hipMalloc(&c->d_tbase, sizeof(int)));
    HIPTRY(hipMemset(c->d_tbase, 0, sizeof(int)));
    HIPTRY(hipEventCreateWithFlags(&c->gev_main, hipEventDisableTiming));
    HIPTRY(hipEventCreateWithFlags(&c->gev_edge, hipEventDisableTiming));
    HIPTRY(hipEventCreateWithFlags(&c->gev_comm, hipEventDisableTiming));
    HIPTRY(hipMalloc(&c->d_solid_count, sizeof(int)));
    HIPTRY(hipMalloc(&c->d_maxbits, sizeof(unsigned long long)));
    HIPTRY(hipMalloc(&c->d_force_now, 3 * sizeof(double)));
    HIPTRY(hipMalloc(&c->d_feq, Q * sizeof(double)));
    if (p->precision == LBM_PRECISION_F32) {
        float v[Q];
        for (int i = 0; i < Q; ++i) v[i] = (float)c->feq_in[i];
        HIPTRY(hipMemcpy(c->d_feq, v, sizeof(v), hipMemcpyHostToDevice));
    } else {
        HIPTRY(hipMemcpy(c->d_feq, c->feq_in, Q * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPTRY(hipMalloc(&c->d_urow, (size_t)p->ny * c->esize));   // the uniform inflow until lbm_set_inlet_profile replaces it
    {
        c->h_urow.assign((size_t)p->ny, p->inlet_velocity);
        if (int rc = upload_rows(c, c->d_urow, c->h_urow.data(), c->h_urow.size())) return bail(rc);
    }
    HIPTRY(c->force_log.alloc(3, c->log_cap, false));
    HIPTRY(hipMalloc(&c->d_halo, 4 * HR1 * Q * sizeof(double) * (size_t)c->nx));
    HIPTRY(hipMalloc(&c->d_red, 64 * sizeof(double)));
#undef HIPTRY
    *out = c;
    return LBM_OK;
}

void lbm_destroy(lbm_ctx* c) {
    if (!c) return;
    lbm_trace("destroy", "ctx %p begin", (void*)c);
    (void)hipSetDevice(c->device);
    // A group that ran into LBM_ERR_TIMEOUT: its threads may still be inside a runtime call on this context's streams. Wait for them
    // (bounded); if they never come back, or the streams never drain, the context is LEAKED — freeing it under a thread that may still
    // wake up, or blocking for ever in a drain, would turn a reported error into a crash or a hang.
    bool leak = c->pool && c->pool->S->broken.load() && !c->pool->quiesce(std::max(5000L, c->pool->S->timeout_ms));
    if (!leak && c->stream && wait_stream(c, c->stream, "compute stream (lbm_destroy)") == LBM_ERR_TIMEOUT) leak = true;
    if (!leak && c->comm_stream && wait_stream(c, c->comm_stream, "exchange stream (lbm_destroy)") == LBM_ERR_TIMEOUT) leak = true;
    if (!leak && c->split_stream && wait_stream(c, c->split_stream, "second compute stream (lbm_destroy)") == LBM_ERR_TIMEOUT) leak = true;
    for (lbm_ctx* nb : {c->nb_south, c->nb_north, c->ring_south, c->ring_north}) {  // a destroyed member leaves its group
        if (!nb || nb == c) continue;
        // the neighbour's exchange stream may still hold a pull (hipMemcpyPeerAsync) that READS this member's edge rows, and
        // freeing a buffer only waits for work of this member's own device: drain the neighbour's streams first
        (void)hipSetDevice(nb->device);
        if (!leak && nb->comm_stream && wait_stream(nb, nb->comm_stream, "a neighbour's exchange stream (lbm_destroy)") == LBM_ERR_TIMEOUT) leak = true;
        if (!leak && nb->stream && wait_stream(nb, nb->stream, "a neighbour's compute stream (lbm_destroy)") == LBM_ERR_TIMEOUT) leak = true;
        if (nb->nb_south == c) nb->nb_south = nullptr;
        if (nb->nb_north == c) nb->nb_north = nullptr;
        if (nb->ring_south == c) nb->ring_south = nullptr;
        if (nb->ring_north == c) nb->ring_north = nullptr;
    }
    (void)hipSetDevice(c->device);
    if (leak) {
        fprintf(stderr, "lbm_destroy: context %p left allocated (%s)\n", (void*)c, g_err);
        lbm_trace("destroy", "ctx %p LEAKED: %s", (void*)c, g_err);
        c->nb_south = c->nb_north = c->ring_south = c->ring_north = nullptr;
        return;
    }
    // (a graph that captured RCCL operations holds the communicator: ncclCommDestroy waits for it to go away first)
    if (c->gexec) { (void)hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->comm) { lbm_trace("destroy", "ctx %p ncclCommDestroy", (void*)c); ncclCommDestroy(c->comm); }
    c->pool.reset();
    void* ptrs[] = {c->buf[0], c->buf[1], c->scratch, c->d_macro, c->d_maxbits, c->d_unstable, c->d_tbase, c->d_solid_count, c->d_feq,
                    c->d_force_now, c->force_log.d, c->d_halo, c->d_red, (void*)c->mview.bits, (void*)c->mview.sat, c->d_fpart,
                    c->d_urow, c->d_feqrow, c->d_sched, c->d_wpx, c->d_urow0, c->d_stats, c->d_labels, c->d_body_box, c->d_body_chunks, c->d_body_first, c->d_body_part,
                    c->d_body_now, c->body_log.d, c->frames.d, c->d_probe_table, c->probes.d};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    hipEvent_t evs[] = {c->ev_edge, c->ev_comm, c->ev_main, c->ev_t0, c->ev_t1, c->gev_main, c->gev_edge, c->gev_comm};
    for (hipEvent_t e : evs)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->split_stream) (void)hipStreamDestroy(c->split_stream);
    lbm_trace("destroy", "ctx %p end", (void*)c);
    delete c;
}

namespace {
// May this context run deep shape `deep` under collision model `collision` (deep_refusal, lbm_plan.hpp)? `settled`: its arithmetic mode
// and its extent count too (lbm_initialise: the arithmetic and the strip options may follow `deep`).
int refuse_deep(const lbm_ctx* c, int collision, int deep, bool settled) {
    const bool whole = !((c->comm && c->nranks > 1) || c->group_n > 1 || c->loopback || c->periodic_y || c->nyl != c->p.ny);
    const std::string why = deep_refusal(deep, (int)c->esize, collision_model(collision), settled, c->arith == AR_CONTRACTED, whole);
    return why.empty() ? LBM_OK : fail(LBM_ERR_ARG, "%s", why.c_str());
}
// What the setters of the collision models share once the value is accepted. A nonzero value (value2: the second one of a model with
// two, the force's Fy): the model `base` with that parameter, unless
// the context has another model (`what`: the caller's name and its word for the value) or, where the setter checks it (`tall_now`), is
// pinned to tall regions the model lacks; 0 (both): that model off, the BGK kernels.
int set_collision(lbm_ctx* c, int base, double value, const char* what, bool tall_now, double value2 = 0.0) {
    const CollisionModel& cur = collision_model(c->collision);
    const bool on = value != 0.0 || value2 != 0.0;      // (Cs and the magic parameter are never negative: their setters refuse that)
    if (on && c->collision != base && c->collision != AR_STRICT)
        return fail(LBM_ERR_ARG, "%s %s on a context with %s %s%s (the two collisions cannot be combined)", what, param_text(collision_model(base), value, value2).c_str(),
                    cur.param, cur.value, param_text(cur, c->collision_param, c->collision_param2).c_str());
    if (on && tall_now) { if (int rc = refuse_deep(c, base, c->deep, false)) return rc; }
    if (on) { c->collision = base; c->collision_param = value; c->collision_param2 = value2; }
    else if (c->collision == base) { c->collision = AR_STRICT; c->collision_param = 0.0; c->collision_param2 = 0.0; }
    return LBM_OK;
}
// ---- the outlet sponge (lbm_set_sponge) ----
// The relaxation time of column x: tau up to x0 = nx - 1 - width, then tau + (tau_end - tau) s^2 with s = (x - x0) / width, every
// operation in double and in this order (no contraction: the Python sponge_tau forms the same bits).
double sponge_tau_at(int nx, double tau, int width, double tau_end, int x) {
#pragma clang fp contract(off)
    const int x0 = nx - 1 - width;
    if (width <= 0 || x <= x0) return tau;
    const double s = (double)(x - x0) / (double)width;
    const double s2 = s * s;
    const double rise = (tau_end - tau) * s2;
    return tau + rise;
}
double sponge_tau_of(const lbm_ctx* c, int x) {
    const bool on = c->collision == AR_STRICT_SPONGE;
    return sponge_tau_at(c->nx, c->p.tau, on ? (int)c->collision_param : 0, c->collision_param2, x);
}
// the rate of column x as the kernels see it, (double)(T)(1 / tau_x)
double sponge_rate_at(const lbm_ctx* c, int x) {
    const double wp = 1.0 / sponge_tau_of(c, x);
    return c->esize == 4 ? (double)(float)wp : wp;
}
// lbm_initialise on a sponge context: the table KArgs::wp_x of all nx columns, cast once; no table on any other context
int upload_sponge(lbm_ctx* c) {
    if (c->d_wpx) { HIPCHK(hipFree(c->d_wpx)); c->d_wpx = nullptr; }
    if (c->collision != AR_STRICT_SPONGE) return LBM_OK;
    std::vector<double> wp((size_t)c->nx);
    for (int x = 0; x < c->nx; ++x) wp[(size_t)x] = 1.0 / sponge_tau_of(c, x);
    HIPCHK(hipMalloc(&c->d_wpx, wp.size() * c->esize));
    return upload_rows(c, c->d_wpx, wp.data(), wp.size());
}
}  // namespace

int lbm_initialise(lbm_ctx* c, int* solid_count_out) {
    if (!c) return fail(LBM_ERR_ARG, "null context");
    lbm_trace("initialise", "ctx %p %dx%d rows %d..%d begin", (void*)c, c->nx, c->p.ny, c->p.y_start, c->p.y_start + c->nyl);
    if (int rc = refuse_deep(c, c->collision, c->deep, true)) return rc;
    // a west pressure port solves for the velocity: it takes none (the three settings are known only here)
    if (c->port_kind[0] == LBM_PORT_PRESSURE && c->has_profile)
        return fail(LBM_ERR_ARG, "lbm_initialise: an inlet profile (lbm_set_inlet_profile) with a west pressure port (lbm_set_port): a pressure port takes no inlet velocity");
    if (c->port_kind[0] == LBM_PORT_PRESSURE && c->has_sched())
        return fail(LBM_ERR_ARG, "lbm_initialise: an inlet schedule (lbm_set_inlet_schedule) with a west pressure port (lbm_set_port): a pressure port takes no inlet velocity");
    if (c->periodic_y) { if (int rc = refuse_periodic(c)) return rc; }
    HIPCHK(hipSetDevice(c->device));
    if (c->periodic_y) { if (int rc = prepare_periodic(c)) return rc; }
    if (c->has_sched()) { if (int rc = prepare_schedule(c)) return rc; }
    { int wr = wait_stream(c, c->stream, "compute stream (lbm_initialise)"); if (wr) return wr; }
    if (int rc = upload_sponge(c)) return rc;       // (behind the wait: a launch in flight may read the table this replaces)        // (re-)initialisation starts from quiet streams
    { int wr = wait_stream(c, c->comm_stream, "exchange stream (lbm_initialise)"); if (wr) return wr; }
    { int wr = wait_stream(c, c->split_stream, "second compute stream (lbm_initialise)"); if (wr) return wr; }
    c->split_i = 0;
    c->steps_done = 0;
    c->force_log.ix.reset(); c->body_log.ix.reset(); c->frames.ix.reset(); c->probes.ix.reset();
    c->mid_pair = false;
    c->comm_issued = false;
    c->ext_split_pending = false;
    graph_drop(c);                 // (a captured graph holds the addresses of the buffers this call is about to replace)
    c->graph_failed = false;
    c->graph_note[0] = 0;
    if (c->scratch) { (void)hipFree(c->scratch); c->scratch = nullptr; }
    int rc = DISPATCH(c, do_initialise<double>(c), do_initialise<float>(c));
    if (rc) return rc;
    int sc = 0;
    HIPCHK(hipMemcpyAsync(&sc, c->d_solid_count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (solid_count_out) *solid_count_out = sc;
    c->initialised = true;
    lbm_trace("initialise", "ctx %p end: %s", (void*)c, c->plan_desc);
    if (c->stats_opt >= 0) { int sr = lbm_stats_begin(c, c->stats_opt); if (sr) return sr; }      // option "stats" (the plan was measured without it)
    if (c->frames_opt > 0) return lbm_frames_begin(c, c->frames_opt, LBM_FRAMES_DEFAULT_CAPACITY);  // option "frames", likewise
    return LBM_OK;
}

int lbm_step(lbm_ctx* c, int nsteps, int output_frequency) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    if (nsteps < 0) return fail(LBM_ERR_ARG, "nsteps < 0");
    if (c->group_n > 1) return fail(LBM_ERR_ARG, "this context is a member of a group: use lbm_group_step");
    HIPCHK(hipSetDevice(c->device));
    lbm_trace("step", "ctx %p t=%d +%d begin", (void*)c, c->steps_done, nsteps);
    const int rc = DISPATCH(c, do_steps<double>(&c, 1, nsteps, output_frequency), do_steps<float>(&c, 1, nsteps, output_frequency));
    lbm_trace("step", "ctx %p t=%d issued rc=%d", (void*)c, c->steps_done, rc);
    return rc;
}

int lbm_sync(lbm_ctx* c) {
    if (!c) return fail(LBM_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    // bounded (a poll) where the caller has set "wait_timeout_ms"; else the blocking call, which a watchdog names if it stalls (lbm_ctx.hpp)
    auto wait = [&](hipStream_t s, const char* what) { return c->wait_timeout_ms > 0 ? wait_stream(c, s, what) : sync_stream_blocking(c, s, what); };
    int rc = wait(c->stream, "compute stream");
    if (!rc) rc = wait(c->comm_stream, "exchange stream");
    if (!rc) rc = wait(c->split_stream, "second compute stream");      // (a call joins it into the compute stream before it returns: empty by now)
    return rc;
}

int lbm_steps_done(const lbm_ctx* c) { return c ? c->steps_done : -1; }

int lbm_first_unstable_step(lbm_ctx* c, int* t_out) {
    if (!c || !t_out) return fail(LBM_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    int v = INT_MAX;
    HIPCHK(hipMemcpyAsync(&v, c->d_unstable, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *t_out = (v == INT_MAX) ? -1 : v;
    return LBM_OK;
}

int lbm_get_forces(lbm_ctx* c, double* fx, double* fy) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    int rc = DISPATCH(c, launch_forces<double>(c, c->d_force_now, c->steps_done),
                      launch_forces<float>(c, c->d_force_now, c->steps_done));
    if (rc) return rc;
    double h[3];
    HIPCHK(hipMemcpyAsync(h, c->d_force_now, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (fx) *fx = h[1];
    if (fy) *fy = h[2];
    return LBM_OK;
}

int lbm_drain_force_log(lbm_ctx* c, lbm_force_row* rows, int max_rows) {
    if (!c || (!rows && max_rows > 0)) return fail(LBM_ERR_ARG, "null argument");
    const int n = c->force_log.ix.count;
    if (max_rows < n) return fail(LBM_ERR_ARG, "force log holds %d rows, buffer takes %d", n, max_rows);
    return drain_force_rows(c, c->force_log, 1, rows, n, [](lbm_force_row& r, size_t, int t) { r.timestep = t; });
}

/* ---- per-body forces (lbm_set_body_labels): k_forces_bodies over the chunk table of the bodies' boxes ---- */
int lbm_body_count(const lbm_ctx* c) { return c ? c->body_n : 0; }

int lbm_get_body_forces(lbm_ctx* c, double* fxy) {
    if (!c || !c->initialised || !fxy) return fail(LBM_ERR_ARG, "lbm_get_body_forces needs an initialised context and an output array");
    if (c->body_n < 1) return fail(LBM_ERR_ARG, "lbm_get_body_forces: this context has no body labels (lbm_set_body_labels)");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    int rc = DISPATCH(c, launch_body_forces<double>(c, c->d_body_now, c->steps_done), launch_body_forces<float>(c, c->d_body_now, c->steps_done));
    if (rc) return rc;
    std::vector<double> h(3 * (size_t)c->body_n);
    HIPCHK(hipMemcpyAsync(h.data(), c->d_body_now, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int b = 0; b < c->body_n; ++b) { fxy[2 * b] = h[3 * (size_t)b + 1]; fxy[2 * b + 1] = h[3 * (size_t)b + 2]; }
    return LBM_OK;
}

int lbm_drain_body_force_log(lbm_ctx* c, lbm_body_force_row* rows, int max_rows) {
    if (!c || (!rows && max_rows > 0)) return fail(LBM_ERR_ARG, "null argument");
    if (c->body_n < 1 || max_rows < c->body_n || c->body_log.ix.count < 1) return 0;       // whole samples only
    const int B = c->body_n;
    const int n = drain_force_rows(c, c->body_log, B, rows, max_rows / B, [B](lbm_body_force_row& r, size_t k, int t) { r.timestep = t; r.body = (int)(k % B) + 1; });
    return n < 0 ? n : B * n;
}

int lbm_get_macros(lbm_ctx* c, double* rho, double* ux, double* uy) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    if (c->last_was_pair || c->restored) return fail(LBM_ERR_ARG, "snapshot unavailable: the previous iteration's populations are not resident (fused trailing launch or restored state); take one more lbm_step(c,1,..)");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    int rc = DISPATCH(c, do_macros<double>(c, false), do_macros<float>(c, false));
    if (rc) return rc;
    const size_t n = (size_t)c->nx * c->nyl;
    if (rho) HIPCHK(hipMemcpyAsync(rho, c->d_macro, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (ux) HIPCHK(hipMemcpyAsync(ux, c->d_macro + n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (uy) HIPCHK(hipMemcpyAsync(uy, c->d_macro + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LBM_OK;
}

int lbm_max_velocity_sq(lbm_ctx* c, double* out) {
    if (!c || !c->initialised || !out) return fail(LBM_ERR_ARG, "bad argument");
    if (c->last_was_pair || c->restored) return fail(LBM_ERR_ARG, "snapshot unavailable: the previous iteration's populations are not resident (fused trailing launch or restored state); take one more lbm_step(c,1,..)");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    int rc = DISPATCH(c, do_macros<double>(c, true), do_macros<float>(c, true));
    if (rc) return rc;
    unsigned long long bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, c->d_maxbits, sizeof(bits), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(out, &bits, sizeof(double));
    return LBM_OK;
}

/* ---- time-averaged statistics: six running sums per cell, sampled at the force-output iterations of lbm_step (k_stats) ---- */
static size_t stats_bytes(const lbm_ctx* c) { return 6 * (size_t)c->nx * c->nyl * sizeof(double); }
// everything queued so far precedes a change of the accumulators made on the compute stream
static int stats_zero(lbm_ctx* c) {
    { int jr = join_comm(c); if (jr) return jr; }
    HIPCHK(hipMemsetAsync(c->d_stats, 0, stats_bytes(c), c->stream));
    c->stats_n = 0;
    return LBM_OK;
}

int lbm_stats_begin(lbm_ctx* c, int from_step) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "lbm_stats_begin needs an initialised context");
    if (from_step < 0) return fail(LBM_ERR_ARG, "from_step < 0");
    HIPCHK(hipSetDevice(c->device));
    if (!c->d_stats && hipMalloc(&c->d_stats, stats_bytes(c)) != hipSuccess) {
        (void)hipGetLastError();
        c->d_stats = nullptr;
        return fail(LBM_ERR_ALLOC, "statistics: no device memory for %zu bytes of accumulators", stats_bytes(c));
    }
    int rc = stats_zero(c);
    if (rc) return rc;
    c->stats_from = from_step;
    c->stats_active = true;
    return LBM_OK;
}

int lbm_stats_end(lbm_ctx* c) {
    if (!c) return fail(LBM_ERR_ARG, "null context");
    c->stats_active = false;
    return LBM_OK;
}

int lbm_stats_samples(const lbm_ctx* c) { return c ? c->stats_n : LBM_ERR_ARG; }

int lbm_get_stat_sums(lbm_ctx* c, double* sums6) {
    if (!c || !sums6) return fail(LBM_ERR_ARG, "null argument");
    if (!c->d_stats) return fail(LBM_ERR_ARG, "statistics were never begun (lbm_stats_begin)");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    HIPCHK(hipMemcpyAsync(sums6, c->d_stats, stats_bytes(c), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LBM_OK;
}

int lbm_stats_restore(lbm_ctx* c, const double* sums6, int samples) {
    if (!c || !c->initialised || !sums6) return fail(LBM_ERR_ARG, "lbm_stats_restore needs an initialised context and the sums");
    if (samples < 0) return fail(LBM_ERR_ARG, "samples < 0");
    if (!c->d_stats) { int rc = lbm_stats_begin(c, 0); if (rc) return rc; }
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    HIPCHK(hipMemcpyAsync(c->d_stats, sums6, stats_bytes(c), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));       // (the caller's array is free again)
    c->stats_n = samples;
    c->stats_active = true;
    return LBM_OK;
}

/* ---- coarsened flow frames: rho, ux, uy and vorticity block-averaged k x k into a device ring at the force-output iterations (k_frame) ---- */
int lbm_frames_begin(lbm_ctx* c, int k, int capacity) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "lbm_frames_begin needs an initialised context");
    if (k < 1 || k > lbmk::FRAME_MAX_K) return fail(LBM_ERR_ARG, "frame stride k = %d outside 1..%d", k, lbmk::FRAME_MAX_K);
    if (capacity < 1) return fail(LBM_ERR_ARG, "frame ring capacity %d < 1", capacity);
    if (c->nx < 2 || c->p.ny < 2) return fail(LBM_ERR_ARG, "frames need nx >= 2 and ny >= 2 (the vorticity differences)");
    if (c->nx % k) return fail(LBM_ERR_ARG, "frame stride k = %d does not divide nx = %d", k, c->nx);
    if (c->p.y_start % k) return fail(LBM_ERR_ARG, "frame stride k = %d does not divide the strip's y_start = %d", k, c->p.y_start);
    if (c->nyl % k) return fail(LBM_ERR_ARG, "frame stride k = %d does not divide the strip's local_ny = %d", k, c->nyl);
    const size_t per = 4 * (size_t)(c->nx / k) * (size_t)(c->nyl / k);
    const int rc = replace_ring(c, c->frames, per, capacity);
    if (rc && rc != LBM_ERR_ALLOC) return rc;
    c->frames_k = k;
    c->frames_active = !rc;
    if (rc) return fail(LBM_ERR_ALLOC, "frames: no device memory for a ring of %d frames (%zu bytes)", capacity, per * sizeof(float) * (size_t)capacity);
    return LBM_OK;
}

int lbm_frames_end(lbm_ctx* c) {
    if (!c) return fail(LBM_ERR_ARG, "null context");
    c->frames_active = false;
    return LBM_OK;
}

int lbm_frames_pending(const lbm_ctx* c) { return c ? c->frames.ix.count : LBM_ERR_ARG; }

int lbm_drain_frames(lbm_ctx* c, int* timesteps, float* frames, int max_frames) {
    if (!c || max_frames < 0 || (max_frames > 0 && !frames)) return fail(LBM_ERR_ARG, "lbm_drain_frames: null argument or max_frames < 0");
    if (c->frames.ix.count < 1 || max_frames < 1) return 0;
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    return c->frames.drain(c->stream, frames, timesteps, max_frames);
}

/* ---- point probes: (rho, ux, uy) interpolated bilinearly at chosen points into a device ring at the force-output iterations (k_probes) ---- */
// The argument checks shared by lbm_probes_begin and lbm_debug_probe_table; the text names the offender.
static int check_probes(const double* xy, int n, int nx, int ny) {
    if (!xy) return fail(LBM_ERR_ARG, "probes: null coordinate array");
    if (n < 1) return fail(LBM_ERR_ARG, "probes: n = %d < 1", n);
    if (n > LBM_PROBES_MAX) return fail(LBM_ERR_ARG, "probes: n = %d > LBM_PROBES_MAX = %d", n, LBM_PROBES_MAX);
    for (int j = 0; j < n; ++j) {
        const double px = xy[2 * j], py = xy[2 * j + 1];
        if (!std::isfinite(px) || !std::isfinite(py)) return fail(LBM_ERR_ARG, "probe %d: (%g, %g) is not finite", j, px, py);
        if (px < 0.0 || px > (double)(nx - 1)) return fail(LBM_ERR_ARG, "probe %d: x = %.17g outside the domain 0..%d", j, px, nx - 1);
        if (py < 0.0 || py > (double)(ny - 1)) return fail(LBM_ERR_ARG, "probe %d: y = %.17g outside the domain 0..%d", j, py, ny - 1);
    }
    return LBM_OK;
}

int lbm_probes_begin(lbm_ctx* c, const double* xy, int n, int capacity) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "lbm_probes_begin needs an initialised context");
    { int cr = check_probes(xy, n, c->nx, c->p.ny); if (cr) return cr; }
    if (capacity < 1) return fail(LBM_ERR_ARG, "probe ring capacity %d < 1", capacity);
    int rc = replace_ring(c, c->probes, 3 * (size_t)n, capacity);
    if (rc && rc != LBM_ERR_ALLOC) return rc;
    // (the sample that was in flight read the old table too)
    if (c->d_probe_table) { (void)hipFree(c->d_probe_table); c->d_probe_table = nullptr; }
    c->probes_active = false;
    c->probe_n = 0;
    std::vector<lbmk::ProbeEntry> table((size_t)n);
    for (int j = 0; j < n; ++j) table[(size_t)j] = lbmk::probe_entry(xy[2 * j], xy[2 * j + 1], c->p.y_start, c->nyl);
    const size_t tbytes = sizeof(lbmk::ProbeEntry) * (size_t)n;
    if (!rc && hipMalloc(&c->d_probe_table, tbytes) != hipSuccess) { (void)hipGetLastError(); c->d_probe_table = nullptr; rc = LBM_ERR_ALLOC; }
    if (rc) {
        c->probes.release();
        return fail(LBM_ERR_ALLOC, "probes: no device memory for a ring of %d samples of %d probes (%zu bytes)", capacity, n, 3 * sizeof(double) * (size_t)n * (size_t)capacity);
    }
    HIPCHK(hipMemcpy(c->d_probe_table, table.data(), tbytes, hipMemcpyHostToDevice));
    c->probe_n = n;
    c->probes_active = true;
    return LBM_OK;
}

int lbm_probes_end(lbm_ctx* c) {
    if (!c) return fail(LBM_ERR_ARG, "null context");
    c->probes_active = false;
    return LBM_OK;
}

int lbm_probes_count(const lbm_ctx* c) { return c ? c->probe_n : LBM_ERR_ARG; }
int lbm_probes_pending(const lbm_ctx* c) { return c ? c->probes.ix.count : LBM_ERR_ARG; }

int lbm_drain_probes(lbm_ctx* c, int* timesteps, double* vals, int max_samples) {
    if (!c || max_samples < 0 || (max_samples > 0 && !vals)) return fail(LBM_ERR_ARG, "lbm_drain_probes: null argument or max_samples < 0");
    if (c->probes.ix.count < 1 || max_samples < 1) return 0;
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    return c->probes.drain(c->stream, vals, timesteps, max_samples);
}

/* TEST HOOK (no device needed): the probe table lbm_probes_begin uploads for the strip [y_start, y_start + local_ny): see include/lbm_hip.h. */
int lbm_debug_probe_table(const double* xy, int n, int nx, int ny, int y_start, int local_ny, int* cells4, double* weights2, int* owned) {
    if (nx < 1 || ny < 1 || y_start < 0 || local_ny < 1 || y_start + local_ny > ny) return fail(LBM_ERR_ARG, "probe table: strip [%d, %d) outside the lattice %dx%d", y_start, y_start + local_ny, nx, ny);
    { int cr = check_probes(xy, n, nx, ny); if (cr) return cr; }
    for (int j = 0; j < n; ++j) {
        const lbmk::ProbeEntry e = lbmk::probe_entry(xy[2 * j], xy[2 * j + 1], y_start, local_ny);
        if (cells4) {      // x1, y1 as k_probes forms them from the entry
            cells4[4 * j] = e.x0; cells4[4 * j + 1] = e.y0;
            cells4[4 * j + 2] = e.x0 + 1 < nx ? e.x0 + 1 : nx - 1;
            cells4[4 * j + 3] = y_start + e.y0 + 1 < ny ? e.y0 + 1 : e.y0;
        }
        if (weights2) { weights2[2 * j] = e.fx; weights2[2 * j + 1] = e.fy; }
        if (owned) owned[j] = e.owned;
    }
    return n;
}

int lbm_get_populations(lbm_ctx* c, int which, double* aos) {
    if (!c || !c->initialised || !aos || (which != 0 && which != 1)) return fail(LBM_ERR_ARG, "bad argument");
    if (c->last_was_pair || c->restored) return fail(LBM_ERR_ARG, "snapshot unavailable: the previous iteration's populations are not resident (fused trailing launch or restored state); take one more lbm_step(c,1,..)");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    return DISPATCH(c, do_populations<double>(c, which, aos), do_populations<float>(c, which, aos));
}

int lbm_set_f_current(lbm_ctx* c, const double* aos) {
    if (!c || !c->initialised || !aos) return fail(LBM_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->comm_stream));
    int rc = DISPATCH(c, do_set_f_current<double>(c, aos), do_set_f_current<float>(c, aos));
    if (rc) return rc;
    if ((c->comm || self_wrap(c)) && c->group_n <= 1)   // (a group: lbm_group_refresh_halos once every member is set)
        rc = DISPATCH(c, exchange_rccl<double>(c, c->cur, c->stream), exchange_rccl<float>(c, c->cur, c->stream));
    return rc;
}

int lbm_get_solid(lbm_ctx* c, unsigned char* mask) {
    if (!c || !mask) return fail(LBM_ERR_ARG, "null argument");
    if (c->has_mask) {
        const MaskView m = c->hmask.view();
        for (int y = 0; y < c->nyl; ++y)
            for (int x = 0; x < c->nx; ++x) mask[(size_t)y * c->nx + x] = mask_cell(m, x, c->p.y_start + y) ? 1 : 0;
        return LBM_OK;
    }
    const double r2 = (double)(c->cyl_r * c->cyl_r);
    for (int y = 0; y < c->nyl; ++y)
        for (int x = 0; x < c->nx; ++x) {
            const double dx = x - c->cyl_x, dy = (c->p.y_start + y) - c->cyl_y;
            mask[(size_t)y * c->nx + x] = (dx * dx + dy * dy <= r2) ? 1 : 0;
        }
    return LBM_OK;
}

int lbm_set_solid_mask(lbm_ctx* c, const unsigned char* mask, int nx, int ny) {
    if (!c || !mask) return fail(LBM_ERR_ARG, "lbm_set_solid_mask: null argument");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_solid_mask must be called before lbm_initialise");
    if (nx != c->nx || ny != c->p.ny) return fail(LBM_ERR_ARG, "lbm_set_solid_mask: mask is %dx%d, the domain %dx%d", nx, ny, c->nx, c->p.ny);
    HostMask h = pack_mask(mask, nx, ny, c->p.y_start, c->nyl);
    HIPCHK(hipSetDevice(c->device));
    {   // a mask replaces the geometry wholesale: the labels of an earlier lbm_set_body_labels go with it
        void** q[] = {(void**)&c->d_labels, (void**)&c->d_body_box, (void**)&c->d_body_chunks, (void**)&c->d_body_first, (void**)&c->d_body_part,
                      (void**)&c->d_body_now};
        for (void** d : q)
            if (*d) { HIPCHK(hipFree(*d)); *d = nullptr; }
        c->body_n = c->body_chunks = 0;
        c->body_log.release();
    }
    c->has_mask = false;
    if (int rc = upload_mask(c, h)) return rc;
    c->hmask = std::move(h);
    c->user_mask = wrapped_rows(mask, nx, ny, c->p.y_start, c->nyl);      // (periodic y: lbm_initialise builds the wrapped window from them)
    c->has_mask = true;
    return LBM_OK;
}

int lbm_set_body_labels(lbm_ctx* c, const unsigned char* labels, int nx, int ny) {
    if (!c || !labels) return fail(LBM_ERR_ARG, "lbm_set_body_labels: null argument");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_body_labels must be called before lbm_initialise");
    if (nx != c->nx || ny != c->p.ny) return fail(LBM_ERR_ARG, "lbm_set_body_labels: labels are %dx%d, the domain %dx%d", nx, ny, c->nx, c->p.ny);
    int rc = lbm_set_solid_mask(c, labels, nx, ny);      // the geometry: nonzero = solid (clears labels set earlier)
    if (rc) return rc;
    const HostBodies h = pack_bodies(labels, nx, ny, c->p.y_start, c->nyl);
    if (h.B < 1) return LBM_OK;                          // no solid cell: no body, nothing to report
    const size_t nch = h.chunks.size();
    HIPCHK(hipMalloc(&c->d_labels, h.lab.size()));
    HIPCHK(hipMalloc(&c->d_body_box, h.box.size() * sizeof(int)));
    HIPCHK(hipMalloc(&c->d_body_chunks, std::max<size_t>(1, nch) * sizeof(BodyChunk)));
    HIPCHK(hipMalloc(&c->d_body_first, h.first.size() * sizeof(int)));
    HIPCHK(hipMalloc(&c->d_body_part, std::max<size_t>(1, nch) * 2 * sizeof(double)));
    HIPCHK(hipMalloc(&c->d_body_now, 3 * sizeof(double) * (size_t)h.B));
    HIPCHK(c->body_log.alloc(3 * (size_t)h.B, c->log_cap, false));
    HIPCHK(hipMemcpy(c->d_labels, h.lab.data(), h.lab.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_body_box, h.box.data(), h.box.size() * sizeof(int), hipMemcpyHostToDevice));
    if (nch) HIPCHK(hipMemcpy(c->d_body_chunks, h.chunks.data(), nch * sizeof(BodyChunk), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->d_body_first, h.first.data(), h.first.size() * sizeof(int), hipMemcpyHostToDevice));
    c->body_chunks = (int)nch;
    c->body_n = h.B;                                     // (last: a failure above leaves a context without labels, its buffers to lbm_destroy)
    return LBM_OK;
}

int lbm_set_inlet_profile(lbm_ctx* c, const double* u, int ny) {
    if (!c || !u) return fail(LBM_ERR_ARG, "lbm_set_inlet_profile: null argument");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_inlet_profile must be called before lbm_initialise");
    if (ny != c->p.ny) return fail(LBM_ERR_ARG, "lbm_set_inlet_profile: %d rows given, the domain has %d", ny, c->p.ny);
    for (int y = 0; y < ny; ++y)   // the Zou-He inlet divides by 1 - u
        if (!std::isfinite(u[y]) || u[y] >= 1.0)
            return fail(LBM_ERR_ARG, "lbm_set_inlet_profile: row %d has velocity %g (finite values below 1 only)", y, u[y]);
    HIPCHK(hipSetDevice(c->device));
    c->has_profile = false;
    if (int rc = upload_feqrow(c, u, ny)) return rc;
    if (int rc = upload_rows(c, c->d_urow, u, (size_t)ny)) return rc;
    c->h_urow.assign(u, u + ny);
    c->prof_digest = profile_digest(u, ny);
    c->has_profile = true;
    return LBM_OK;
}

int lbm_set_smagorinsky(lbm_ctx* c, double cs) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_smagorinsky: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_smagorinsky must be called before lbm_initialise");
    if (!std::isfinite(cs) || cs < 0.0 || cs > 1.0) return fail(LBM_ERR_ARG, "lbm_set_smagorinsky: Cs = %g (finite values in [0, 1] only)", cs);
    return set_collision(c, AR_STRICT_LES, cs, "lbm_set_smagorinsky: Cs =", false);    // (pinned to deep 8: lbm_initialise refuses, as it always has)
}

int lbm_set_trt(lbm_ctx* c, double magic) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_trt: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_trt must be called before lbm_initialise");
    if (!std::isfinite(magic) || magic < 0.0 || magic > 1.0)
        return fail(LBM_ERR_ARG, "lbm_set_trt: magic parameter = %g (finite values in [0, 1] only)", magic);
    if (magic > 0.0 && !(c->p.tau > 0.5)) return fail(LBM_ERR_ARG, "lbm_set_trt: tau = %g (the magic parameter needs tau > 0.5)", c->p.tau);
    return set_collision(c, AR_STRICT_TRT, magic, "lbm_set_trt: magic parameter", true);
}

int lbm_set_forcing(lbm_ctx* c, double fx, double fy) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_forcing: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_forcing must be called before lbm_initialise");
    if (!std::isfinite(fx) || !(std::fabs(fx) < 1.0)) return fail(LBM_ERR_ARG, "lbm_set_forcing: fx = %g (finite values of magnitude below 1 only)", fx);
    if (!std::isfinite(fy) || !(std::fabs(fy) < 1.0)) return fail(LBM_ERR_ARG, "lbm_set_forcing: fy = %g (finite values of magnitude below 1 only)", fy);
    return set_collision(c, AR_STRICT_FORCED, fx, "lbm_set_forcing: force", true, fy);
}

int lbm_get_forcing(const lbm_ctx* c, double* fx, double* fy) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_forcing: null context");
    const bool on = c->collision == AR_STRICT_FORCED;
    if (fx) *fx = on ? c->collision_param : 0.0;
    if (fy) *fy = on ? c->collision_param2 : 0.0;
    return LBM_OK;
}

int lbm_set_mrt(lbm_ctx* c, double bulk_rate, double magic) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_mrt: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_mrt must be called before lbm_initialise");
    if (!std::isfinite(bulk_rate) || bulk_rate < 0.0 || bulk_rate >= 2.0)
        return fail(LBM_ERR_ARG, "lbm_set_mrt: bulk rate = %g (0, or finite values in (0, 2) only)", bulk_rate);
    if (!std::isfinite(magic)) return fail(LBM_ERR_ARG, "lbm_set_mrt: magic parameter = %g (finite values only)", magic);
    if (bulk_rate == 0.0) return set_collision(c, AR_STRICT_MRT, 0.0, "lbm_set_mrt:", true, 0.0);
    if (!(magic > 0.0) || magic > 1.0) return fail(LBM_ERR_ARG, "lbm_set_mrt: magic parameter = %g (finite values in (0, 1] only)", magic);
    if (!(c->p.tau > 0.5)) return fail(LBM_ERR_ARG, "lbm_set_mrt: tau = %g (the MRT rates need tau > 0.5)", c->p.tau);
    return set_collision(c, AR_STRICT_MRT, bulk_rate, "lbm_set_mrt: (bulk rate, magic) =", true, magic);
}

int lbm_get_mrt(const lbm_ctx* c, double* bulk_rate, double* magic) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_mrt: null context");
    const bool on = c->collision == AR_STRICT_MRT;
    if (bulk_rate) *bulk_rate = on ? c->collision_param : 0.0;
    if (magic) *magic = on ? c->collision_param2 : 0.0;
    return LBM_OK;
}

int lbm_set_sponge(lbm_ctx* c, int width, double tau_end) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_sponge: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_sponge must be called before lbm_initialise");
    if (width < 0 || width > c->nx - 1)
        return fail(LBM_ERR_ARG, "lbm_set_sponge: width = %d (0 .. nx - 1 = %d only: column 0 keeps tau)", width, c->nx - 1);
    if (width == 0) return set_collision(c, AR_STRICT_SPONGE, 0.0, "lbm_set_sponge:", true, 0.0);
    if (!std::isfinite(tau_end) || !(tau_end > 0.5)) return fail(LBM_ERR_ARG, "lbm_set_sponge: tau_end = %g (finite values above 0.5 only)", tau_end);
    if (!(c->p.tau > 0.5)) return fail(LBM_ERR_ARG, "lbm_set_sponge: tau = %g (the sponge's rates need tau > 0.5)", c->p.tau);
    return set_collision(c, AR_STRICT_SPONGE, (double)width, "lbm_set_sponge: (width, tau_end) =", true, tau_end);
}

int lbm_get_sponge(const lbm_ctx* c, int* width, double* tau_end) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_sponge: null context");
    const bool on = c->collision == AR_STRICT_SPONGE;
    if (width) *width = on ? (int)c->collision_param : 0;
    if (tau_end) *tau_end = on ? c->collision_param2 : 0.0;
    return LBM_OK;
}

int lbm_get_sponge_rate(const lbm_ctx* c, int x, double* wp_out) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_sponge_rate: null context");
    if (!wp_out) return fail(LBM_ERR_ARG, "lbm_get_sponge_rate: null pointer");
    if (x < 0 || x >= c->nx) return fail(LBM_ERR_ARG, "lbm_get_sponge_rate: x = %d (columns 0 .. %d only)", x, c->nx - 1);
    *wp_out = sponge_rate_at(c, x);
    return LBM_OK;
}

int lbm_set_wall(lbm_ctx* c, int side, int kind, double velocity) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_wall: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_wall must be called before lbm_initialise");
    if (int rc = check_wall("lbm_set_wall", side, kind, velocity)) return rc;
    c->wall_kind[side] = kind;
    c->wall_u[side] = kind == LBM_WALL_MOVING ? velocity : 0.0;
    return LBM_OK;
}

int lbm_get_wall(const lbm_ctx* c, int side, int* kind, double* velocity) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_wall: null context");
    if (side != LBM_WALL_SOUTH && side != LBM_WALL_NORTH) return fail(LBM_ERR_ARG, "lbm_get_wall: side = %d (0 south or 1 north only)", side);
    if (kind) *kind = c->wall_kind[side];
    if (velocity) *velocity = c->wall_u[side];
    return LBM_OK;
}

int lbm_set_port(lbm_ctx* c, int side, int kind, double value) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_port: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_port must be called before lbm_initialise");
    if (int rc = check_port("lbm_set_port", side, kind, value)) return rc;
    c->port_kind[side] = kind;
    c->port_value[side] = value;
    return LBM_OK;
}

int lbm_get_port(const lbm_ctx* c, int side, int* kind, double* value) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_get_port: null context");
    if (side != LBM_PORT_WEST && side != LBM_PORT_EAST) return fail(LBM_ERR_ARG, "lbm_get_port: side = %d (0 west or 1 east only)", side);
    if (kind) *kind = c->port_kind[side];
    if (value) *value = c->port_value[side];
    return LBM_OK;
}

int lbm_set_periodic_y(lbm_ctx* c, int on) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_periodic_y: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_periodic_y must be called before lbm_initialise");
    if (on != 0 && on != 1) return fail(LBM_ERR_ARG, "lbm_set_periodic_y: on = %d (0 or 1 only)", on);
    c->periodic_y = on;
    return LBM_OK;
}

int lbm_get_periodic_y(const lbm_ctx* c) { return c ? c->periodic_y : 0; }

int lbm_set_inlet_schedule(lbm_ctx* c, const double* s, int n, int mode) {
    if (!c) return fail(LBM_ERR_ARG, "lbm_set_inlet_schedule: null context");
    if (c->initialised) return fail(LBM_ERR_ARG, "lbm_set_inlet_schedule must be called before lbm_initialise");
    if (int rc = check_schedule("lbm_set_inlet_schedule", s, n, mode)) return rc;
    HIPCHK(hipSetDevice(c->device));
    c->sched.clear();
    c->sched_mode = LBM_INLET_HOLD;
    c->sched_digest = 0;
    if (c->d_sched) { HIPCHK(hipFree(c->d_sched)); c->d_sched = nullptr; }
    if (n == 0) return LBM_OK;
    c->sched.assign(s, s + n);
    c->sched_mode = mode;
    c->sched_digest = schedule_digest(s, n, mode);
    const int rc = DISPATCH(c, upload_schedule<double>(c), upload_schedule<float>(c));
    if (rc) { c->sched.clear(); if (c->d_sched) { (void)hipFree(c->d_sched); c->d_sched = nullptr; } }
    return rc;
}

int lbm_inlet_schedule_length(const lbm_ctx* c) { return c ? (int)c->sched.size() : 0; }

int lbm_get_inlet_scale(const lbm_ctx* c, int t, double* s_out) {
    if (!c || !s_out) return fail(LBM_ERR_ARG, "lbm_get_inlet_scale: null argument");
    if (t < 0) return fail(LBM_ERR_ARG, "lbm_get_inlet_scale: t = %d (iterations count from 0)", t);
    *s_out = DISPATCH(c, (double)inlet_scale<double>(c, t), (double)inlet_scale<float>(c, t));
    return LBM_OK;
}

int lbm_comm_unique_id(void* id128) {
    if (!id128) return fail(LBM_ERR_ARG, "null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return LBM_OK;
}

int lbm_comm_init(lbm_ctx* c, int rank, int nranks, const void* id128) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(LBM_ERR_ARG, "bad argument");
    if (c->initialised) return fail(LBM_ERR_ARG, "attach the communicator before lbm_initialise");
    HIPCHK(hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    lbm_trace("comm_init", "ctx %p rank %d of %d begin", (void*)c, rank, nranks);
    NCCLCHK(ncclCommInitRank(&c->comm, nranks, id, rank));
    lbm_trace("comm_init", "ctx %p end", (void*)c);
    c->rank = rank;
    c->nranks = nranks;
    if (nranks > 1 && c->nyl < 2 * HR1) return fail(LBM_ERR_ARG, "a strip with neighbours needs at least %d rows", 2 * HR1);
    return LBM_OK;
}

int lbm_comm_allreduce(lbm_ctx* c, double* vals, int n, int op) {
    if (!c || !vals || n < 1 || n > 64) return fail(LBM_ERR_ARG, "bad argument");
    if (!c->comm) return (c->nranks == 1) ? LBM_OK : fail(LBM_ERR_COMM, "no communicator");
    HIPCHK(hipSetDevice(c->device));
    return allreduce_doubles(c, vals, n, op);
}

int lbm_runtime_versions(int* rccl, int* hip_runtime, int* hip_driver) {
    int v = 0;
    if (rccl) { NCCLCHK(ncclGetVersion(&v)); *rccl = v; }
    if (hip_runtime) { HIPCHK(hipRuntimeGetVersion(&v)); *hip_runtime = v; }
    if (hip_driver) { HIPCHK(hipDriverGetVersion(&v)); *hip_driver = v; }
    return LBM_OK;
}

const char* lbm_strip_schedule(const lbm_ctx* c) {
    if (!c) return "";
    static thread_local char out[1024];
    if (c->graph_failed) snprintf(out, sizeof(out), "%s; launch groups issued call by call (graph capture given up: %s)", c->sched_desc, c->graph_note);
    else if (c->graph_replays > 0) snprintf(out, sizeof(out), "%s; %ld hipGraph replays of %d launch groups", c->sched_desc, c->graph_replays, GRAPH_GROUPS);
    else snprintf(out, sizeof(out), "%s", c->sched_desc);
    return out;
}

int lbm_device_memory(int device, unsigned long long* free_bytes, unsigned long long* total_bytes) {
    size_t f = 0, t = 0;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return LBM_OK;
}

// ---- in-process groups of strips ----------------------------------------------------------------------------
namespace {
int check_group(lbm_ctx** cs, int n, bool linked) {
    if (!cs || n < 1) return fail(LBM_ERR_ARG, "empty group");
    for (int k = 0; k < n; ++k) {
        if (!cs[k]) return fail(LBM_ERR_ARG, "null context in group");
        if (linked && (cs[k]->group_n != n || cs[k]->group_k != k)) return fail(LBM_ERR_ARG, "not the group these contexts were linked as");
    }
    return LBM_OK;
}
}  // namespace

int lbm_group_link(lbm_ctx** cs, int n, int transport) {
    int rc = check_group(cs, n, false);
    if (rc) return rc;
    if (transport != 0 && transport != 1) return fail(LBM_ERR_ARG, "transport must be 0 (peer copies) or 1 (RCCL)");
    for (int k = 0; k < n; ++k) {
        lbm_ctx* c = cs[k];
        if (c->initialised || c->comm || c->group_n > 1) return fail(LBM_ERR_ARG, "link fresh contexts (before lbm_initialise, without a communicator)");
        if (c->p.precision != cs[0]->p.precision || c->nx != cs[0]->nx || c->p.ny != cs[0]->p.ny)
            return fail(LBM_ERR_ARG, "the strips of a group must share nx, ny and the precision");
        const int expect = k == 0 ? 0 : cs[k - 1]->p.y_start + cs[k - 1]->nyl;
        if (c->p.y_start != expect) return fail(LBM_ERR_ARG, "strip %d starts at row %d, expected %d (bottom to top, contiguous)", k, c->p.y_start, expect);
        if (n > 1 && c->nyl < 2 * HR1) return fail(LBM_ERR_ARG, "a strip with neighbours needs at least %d rows", 2 * HR1);
    }
    if (cs[n - 1]->p.y_start + cs[n - 1]->nyl != cs[0]->p.ny) return fail(LBM_ERR_ARG, "the strips do not cover all %d rows", cs[0]->p.ny);
    if (n == 1) return LBM_OK;
    if (transport == 1) {   // one communicator per member, created together (ncclCommInitAll wants distinct devices)
        std::vector<int> devs((size_t)n);
        std::vector<ncclComm_t> comms((size_t)n);
        for (int k = 0; k < n; ++k) devs[(size_t)k] = cs[k]->device;
        NCCLCHK(ncclCommInitAll(comms.data(), n, devs.data()));
        for (int k = 0; k < n; ++k) { cs[k]->comm = comms[(size_t)k]; cs[k]->rank = k; cs[k]->nranks = n; }
    } else {
        for (int k = 0; k < n; ++k) {
            lbm_ctx* c = cs[k];
            HIPCHK(hipSetDevice(c->device));
            for (lbm_ctx* nb : {k > 0 ? cs[k - 1] : nullptr, k + 1 < n ? cs[k + 1] : nullptr, (c->periodic_y && (k == 0 || k + 1 == n)) ? cs[k == 0 ? n - 1 : 0] : nullptr}) {
                if (!nb || nb->device == c->device) continue;
                int can = 0;
                HIPCHK(hipDeviceCanAccessPeer(&can, c->device, nb->device));
                if (can) {
                    const hipError_t e = hipDeviceEnablePeerAccess(nb->device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail(LBM_ERR_HIP, "hipDeviceEnablePeerAccess(%d -> %d): %s", c->device, nb->device, hipGetErrorString(e));
                    (void)hipGetLastError();
                }   // (without peer access hipMemcpyPeerAsync stages through the host)
            }
            // the neighbours' streams wait on these events and read what the kernels before them wrote: system-scope release
            for (hipEvent_t* ev : {&c->ev_edge, &c->ev_comm}) {
                HIPCHK(hipEventDestroy(*ev));
                HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
            }
        }
    }
    std::shared_ptr<GroupPool> pool(new (std::nothrow) GroupPool(n));
    if (!pool) return fail(LBM_ERR_ALLOC, "out of host memory");
    for (int k = 0; k < n; ++k) {
        cs[k]->nb_south = k > 0 ? cs[k - 1] : nullptr;
        cs[k]->nb_north = k + 1 < n ? cs[k + 1] : nullptr;
        cs[k]->ring_south = k == 0 ? cs[n - 1] : nullptr;      // (neighbours where the group is periodic in y: south_of / north_of)
        cs[k]->ring_north = k + 1 == n ? cs[0] : nullptr;
        cs[k]->group_transport = transport;
        cs[k]->group_n = n;
        cs[k]->group_k = k;
        cs[k]->pool = pool;
    }
    return LBM_OK;
}

int lbm_group_initialise(lbm_ctx** cs, int n, int* solid_total) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    int total = 0;
    for (int k = 0; k < n; ++k)
        if (cs[k]->periodic_y != cs[0]->periodic_y) return fail(LBM_ERR_ARG, "strip %d and strip 0 of the group differ in periodic y (lbm_set_periodic_y): set it on every strip", k);
    for (int k = 0; k < n; ++k) {
        int sc = 0;
        rc = lbm_initialise(cs[k], &sc);
        if (rc) return rc;
        total += sc;
    }
    if (solid_total) *solid_total = total;
    if (n > 1) rc = DISPATCH(cs[0], refresh_group_halos<double>(cs, n), refresh_group_halos<float>(cs, n));
    return rc;
}

int lbm_group_step(lbm_ctx** cs, int n, int nsteps, int output_frequency) {
    int rc = check_group(cs, n, true);
    if (rc) return rc;
    if (nsteps < 0) return fail(LBM_ERR_ARG, "nsteps < 0");
    for (int k = 0; k < n; ++k)
        if (!cs[k]->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    lbm_trace("group_step", "%d strips t=%d +%d begin", n, cs[0]->steps_done, nsteps);
    rc = DISPATCH(cs[0], do_steps<double>(cs, n, nsteps, output_frequency), do_steps<float>(cs, n, nsteps, output_frequency));
    lbm_trace("group_step", "%d strips t=%d issued rc=%d", n, cs[0]->steps_done, rc);
    return rc;
}

int lbm_group_refresh_halos(lbm_ctx** cs, int n) {
    int rc = check_group(cs, n, true);
    if (rc || n == 1) return rc;
    return DISPATCH(cs[0], refresh_group_halos<double>(cs, n), refresh_group_halos<float>(cs, n));
}

int lbm_halo_export(lbm_ctx* c, double* south_out, double* north_out) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    if (c->periodic_y) return fail(LBM_ERR_ARG, "lbm_halo_export: a periodic context (lbm_set_periodic_y) exchanges on the device only");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    return DISPATCH(c, do_halo_export<double>(c, south_out, north_out), do_halo_export<float>(c, south_out, north_out));
}

int lbm_halo_import(lbm_ctx* c, const double* south_in, const double* north_in) {
    if (!c || !c->initialised) return fail(LBM_ERR_ARG, "context not initialised");
    if (c->periodic_y) return fail(LBM_ERR_ARG, "lbm_halo_import: a periodic context (lbm_set_periodic_y) exchanges on the device only");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    return DISPATCH(c, do_halo_import<double>(c, south_in, north_in), do_halo_import<float>(c, south_in, north_in));
}

int lbm_save_state(lbm_ctx* c, const char* path) {
    if (!c || !c->initialised || !path) return fail(LBM_ERR_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    { int jr = join_comm(c); if (jr) return jr; }
    FILE* fp = fopen(path, "wb");
    if (!fp) return fail(LBM_ERR_ARG, "cannot open %s for writing", path);
    unsigned char head[LBM_CKPT_HEAD_MAX];
    const size_t n = (size_t)ckpt_serialise(ckpt_head_of(c), head);
    int rc = fwrite(head, 1, n, fp) == n ? LBM_OK : fail(LBM_ERR_ARG, "short write");
    if (!rc) rc = DISPATCH(c, transfer_interior<double>(c, fp, false), transfer_interior<float>(c, fp, false));
    fclose(fp);
    return rc;
}

int lbm_load_state(lbm_ctx* c, const char* path) {
    if (!c || !c->initialised || !path) return fail(LBM_ERR_ARG, "lbm_load_state needs an initialised context");
    HIPCHK(hipSetDevice(c->device));
    // the state is replaced wholesale: nothing of the run so far may still be in flight on either stream
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->comm_stream));
    c->comm_issued = false;
    c->ext_split_pending = false;
    {
        const int big = INT_MAX;
        HIPCHK(hipMemcpyAsync(c->d_unstable, &big, sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    FILE* fp = fopen(path, "rb");
    if (!fp) return fail(LBM_ERR_ARG, "cannot open %s", path);
    unsigned char head[LBM_CKPT_HEAD_MAX];
    lbm_ckpt_head file{};
    int rc = accept_head(path, head, (int)fread(head, 1, sizeof(head), fp), ckpt_head_of(c), &file);      // (> 0: the bytes of the head)
    if (rc > 0) rc = fseek(fp, rc, SEEK_SET) ? fail(LBM_ERR_ARG, "short read") : DISPATCH(c, transfer_interior<double>(c, fp, true), transfer_interior<float>(c, fp, true));
    fclose(fp);
    if (rc) return rc;
    c->steps_done = file.steps_done;
    c->restored = true;
    c->force_log.ix.reset(); c->body_log.ix.reset();
    c->last_was_pair = false;
    c->mid_pair = false;
    if ((c->comm || self_wrap(c)) && c->group_n <= 1)   // (a group: lbm_group_refresh_halos once every member is restored)
        rc = DISPATCH(c, exchange_rccl<double>(c, c->cur, c->stream), exchange_rccl<float>(c, c->cur, c->stream));
    return rc;
}

int lbm_debug_ckpt_save(lbm_ckpt_head* h, const unsigned char* mask, const double* profile, const double* sched, int sched_n, int sched_mode,
                        unsigned char* out, int cap) {
    if (!h || !out || cap < LBM_CKPT_HEAD_MAX) return fail(LBM_ERR_ARG, "lbm_debug_ckpt_save: a head and %d bytes for it", LBM_CKPT_HEAD_MAX);
    if ((mask && (h->nx < 1 || h->ny < 1)) || (profile && h->ny < 1) || (sched && sched_n < 1)) return fail(LBM_ERR_ARG, "lbm_debug_ckpt_save: data without a size");
    if (mask) { h->has_mask = 1; h->mask_digest = mask_digest(mask, h->nx, h->ny); }
    if (profile) { h->has_profile = 1; h->profile_digest = profile_digest(profile, h->ny); }
    if (sched) { h->has_sched = 1; h->sched_digest = schedule_digest(sched, sched_n, sched_mode); }
    return ckpt_serialise(*h, out);
}

int lbm_debug_ckpt_load(const unsigned char* bytes, int n, const lbm_ckpt_head* here, const char* path, int* consumed_out) {
    if (!bytes || n < 0 || !here || !path) return fail(LBM_ERR_ARG, "lbm_debug_ckpt_load: null argument");
    lbm_ckpt_head file{};
    const int rc = accept_head(path, bytes, n, *here, &file);
    if (consumed_out) *consumed_out = rc > 0 ? rc : 0;
    return rc > 0 ? LBM_OK : rc;
}

int lbm_set_option(lbm_ctx* c, const char* key, long value) {
    if (!c || !key) return fail(LBM_ERR_ARG, "null argument");
    const std::string k(key);
    if (c->initialised && (k == "layout" || k == "nt" || k == "ntl" || k == "tune" || k == "pair" || k == "fuse" || k == "pair_ty" || k == "loopback" || k == "deep" || k == "arith"))
        return fail(LBM_ERR_ARG, "option %s must be set before lbm_initialise", key);
    if (k == "timing") c->timing = (int)value;
    else if (k == "alternate") c->alternate = (int)value;
    else if (k == "layout") { c->layout = (int)value ? 1 : 0; c->layout_pinned = true; }
    else if (k == "periodic_y") {   // lbm_set_periodic_y by its key (the dry runs take options only)
        if (value != 0 && value != 1) return fail(LBM_ERR_ARG, "lbm_set_periodic_y: on = %ld (0 or 1 only)", value);
        return lbm_set_periodic_y(c, (int)value);
    }
    else if (k == "sponge") {       // lbm_set_sponge by its key, width `value` with tau_end 1.5 (the dry runs take options only)
        if (value < INT_MIN || value > INT_MAX) return fail(LBM_ERR_ARG, "sponge must be a width that an int holds");
        return lbm_set_sponge(c, (int)value, 1.5);
    }
    else if (k == "nt") c->use_nt = (int)value ? 1 : 0;
    else if (k == "ntl") c->use_ntl = (int)value ? 1 : 0;
    else if (k == "fuse") { if (value < 1 || value > 4) return fail(LBM_ERR_ARG, "fuse must be 1, 2, 3 or 4 (4: tile kernel, no strip faces)"); c->fuse = (int)value; c->deep = 0; }
    else if (k == "deep") {     // the id of a row of deep_shapes (lbm_plan.hpp)
        if (int rc = refuse_deep(c, c->collision, (int)value, false)) return rc;
        c->deep = (int)value;
        if (c->deep) c->fuse = deep_depth(c->deep);
    }
    else if (k == "pair") c->fuse = (int)value ? 2 : 1;
    else if (k == "trailing_pair") c->trailing_pair = (int)value ? 1 : 0;
    else if (k == "xcd") c->xcd = (int)value ? 1 : 0;
    else if (k == "arith") { if (value != 0 && value != 1) return fail(LBM_ERR_ARG, "arith must be 0 (strict) or 1 (contracted)"); c->arith = (int)value; }
    else if (k == "deep_halo") { if (value < 0 || value > 2) return fail(LBM_ERR_ARG, "deep_halo must be 0, 1 or 2"); c->deep_halo = (int)value; c->deep_pinned = true; }
    else if (k == "halo_trim") { if (value != 0 && value != 1) return fail(LBM_ERR_ARG, "halo_trim must be 0 or 1"); c->halo_trim = (int)value; c->trim_pinned = true; }
    else if (k == "skip_exchange") c->skip_exchange = (int)value ? 1 : 0;
    else if (k == "group_threads") c->group_threads = (int)value ? 1 : 0;
    else if (k == "wait_timeout_ms") { if (value < 0) return fail(LBM_ERR_ARG, "wait_timeout_ms must be >= 0 (0: LBM_WAIT_TIMEOUT_MS or five minutes)"); c->wait_timeout_ms = value; }
    else if (k == "debug_fault_launch") c->debug_fault_launch = (int)value;      // TEST ONLY: see lbm_ctx
    else if (k == "debug_fault_point") { if (value < 0 || value > 2) return fail(LBM_ERR_ARG, "debug_fault_point must be 0, 1 or 2"); c->debug_fault_point = (int)value; }
    else if (k == "debug_fault_stall_ms") c->debug_fault_stall_ms = (int)value;
    else if (k == "debug_old_edge_band") c->debug_old_edge_band = (int)value ? 1 : 0;      // TEST ONLY: see lbm_ctx
    else if (k == "debug_skip_pull_wait") c->debug_skip_pull_wait = (int)value ? 1 : 0;    // TEST ONLY: see lbm_ctx
    else if (k == "debug_skip_split_wait") c->debug_skip_split_wait = (int)value ? 1 : 0;  // TEST ONLY: see lbm_ctx
    else if (k == "split_min") { if (value < 1) return fail(LBM_ERR_ARG, "split_min must be >= 1"); c->split_min = (int)value; }
    else if (k == "split") {    // a whole-domain deep launch of the register family as 3 / 4 staggered row-range launches on two streams (0: one launch)
        if (value != 0 && value != 3 && value != 4) return fail(LBM_ERR_ARG, "split must be 0, 3 or 4");
        c->split = (int)value; c->split_pinned = true;      // (between calls nothing is in flight on the second stream: do_steps joins it)
    }
    else if (k == "stats") {    // statistics from this step on: lbm_stats_begin now, or — not yet initialised — at the end of lbm_initialise
        if (value < 0) return fail(LBM_ERR_ARG, "stats (the first step sampled) must be >= 0");
        if (c->initialised) return lbm_stats_begin(c, (int)value);
        c->stats_opt = (int)value;
    }
    else if (k == "frames") {   // frames of stride K from now on: lbm_frames_begin(c, K, default capacity) now, or — not yet initialised — at the end of lbm_initialise
        if (value < 1 || value > lbmk::FRAME_MAX_K) return fail(LBM_ERR_ARG, "frames (the stride k) must be in 1..%d", lbmk::FRAME_MAX_K);
        if (c->initialised) return lbm_frames_begin(c, (int)value, LBM_FRAMES_DEFAULT_CAPACITY);
        c->frames_opt = (int)value;
    }
    else if (k == "probes") c->probes_opt = (int)value ? 1 : 0;      // dry run only (lbm_debug_choreography): a probe sample behind every force kernel
    else if (k == "bodies") c->bodies_opt = (int)value ? 1 : 0;      // dry run only (lbm_debug_choreography): a body-force sample behind every force kernel
    else if (k == "graph") { if (value < 0 || value > 2) return fail(LBM_ERR_ARG, "graph must be 0, 1 or 2"); c->use_graph = (int)value; }
    else if (k == "loopback") c->loopback = (int)value;   // 0 off, 1 device copies, 2 RCCL self send/recv
    else if (k == "pair_ty") { if (value != 8 && value != 12) return fail(LBM_ERR_ARG, "pair_ty must be 8 or 12"); c->pair_ty = (int)value; }
    else if (k == "tune") c->tune = (int)value ? 1 : 0;
    else if (k == "overlap") { if (value < 0 || value > 2) return fail(LBM_ERR_ARG, "overlap must be 0, 1 or 2"); c->overlap = (int)value; c->overlap_pinned = true; }
    else return fail(LBM_ERR_ARG, "unknown option %s", key);
    return LBM_OK;
}

int lbm_last_step_kernel_ms(lbm_ctx* c, double* ms_per_launch) {
    if (!c || !ms_per_launch) return fail(LBM_ERR_ARG, "null argument");
    *ms_per_launch = 0.0;
    if (!c->timing || c->timed_launches <= 0) return LBM_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_t1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    *ms_per_launch = (double)ms / c->timed_launches;
    return LBM_OK;
}

int lbm_last_step_stats(lbm_ctx* c, double* ms_total, int* launches, int* iterations) {
    if (!c) return fail(LBM_ERR_ARG, "null argument");
    if (ms_total) *ms_total = 0.0;
    if (launches) *launches = c->timed_launches;
    if (iterations) *iterations = c->timed_steps;
    if (!c->timing || c->timed_launches <= 0) return LBM_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_t1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    if (ms_total) *ms_total = (double)ms;
    return LBM_OK;
}

int lbm_last_step_dispatches(const lbm_ctx* c) { return c ? c->timed_dispatches : 0; }

long lbm_graph_replays(const lbm_ctx* c) { return c ? c->graph_replays : 0; }

const char* lbm_kernel_name(const lbm_ctx* c) {
    if (!c) return "";
    static thread_local char name[96];
    // the kernel plan_launch really issues: a strip whose halos are staged through the host carries LBM_HALO_ROWS ghost
    // rows per exchange, so a deeper plan (seven / eight iterations per launch) falls back to the three-iteration tile kernel there
    const bool phys_face = face_south(c) || face_north(c);
    const bool usable = c->deep && (!phys_face || deep_depth(c->deep) <= (device_transport(c) ? GR : HR1));
    const int deep = usable ? c->deep : 0, fuse = usable || !c->deep ? c->fuse : std::min(c->fuse, 3);
    snprintf(name, sizeof(name), "%s", plan_kernel_name(fuse, deep, c->pair_ty, c->use_nt, c->collision | (c->arith == AR_CONTRACTED ? 1 : 0), (int)c->esize).c_str());
    return name;
}

/* TEST HOOK (no device needed): the host-side packing of lbm_set_solid_mask for the strip [y_start, y_start + local_ny) (csrc/lbm_geom.hpp)
 * and the kernels' block-uniform near-solid query over it (lbm_kernels.hpp mask_box_any, the same function the device runs). */
int lbm_debug_geometry(const unsigned char* mask, int nx, int ny, int y_start, int local_ny, int* dims9, unsigned long long* bits, long bits_cap,
                       int* sat, long sat_cap, const int* boxes4, int nbox, int* near_out) {
    if (!mask || !dims9 || nx < 1 || ny < 1 || y_start < 0 || local_ny < 1 || y_start + local_ny > ny || nbox < 0 || (nbox > 0 && (!boxes4 || !near_out)))
        return fail(LBM_ERR_ARG, "bad argument");
    const HostMask h = pack_mask(mask, nx, ny, y_start, local_ny);
    const int d[9] = {h.y0, h.rows, h.words, h.nbx, h.nby, h.bx0, h.bx1, h.by0, h.by1};
    memcpy(dims9, d, sizeof(d));
    if (bits) {
        if (bits_cap < (long)h.bits.size()) return fail(LBM_ERR_ARG, "bits: %zu words needed", h.bits.size());
        memcpy(bits, h.bits.data(), h.bits.size() * sizeof(unsigned long long));
    }
    if (sat) {
        if (sat_cap < (long)h.sat.size()) return fail(LBM_ERR_ARG, "sat: %zu entries needed", h.sat.size());
        memcpy(sat, h.sat.data(), h.sat.size() * sizeof(int));
    }
    const MaskView m = h.view();
    for (int k = 0; k < nbox; ++k) near_out[k] = mask_box_any(m, boxes4[4 * k], boxes4[4 * k + 1], boxes4[4 * k + 2], boxes4[4 * k + 3]) ? 1 : 0;
    return LBM_OK;
}

/* TEST HOOK (no device needed): the per-wave verdict of k_stepc_col (lbm_kernels.hpp wave_plain, the function the kernel's branch calls)
 * for one wave of one tile of one launch of a context that is described, not created: see include/lbm_hip.h. The arguments the kernel
 * would receive are formed as make_kargs, launch_fused_rows and band_origin form them. */
int lbm_debug_wave_plain(int nx, int ny, int y_start, int local_ny, int precision, int arith, int periodic_y, const unsigned char* mask,
                         const double* cylinder3, int deep, int depth, int y_lo, int y_cnt, int bx, int by, int wave, int* dims4) {
    if (nx < 1 || ny < 1 || y_start < 0 || local_ny < 1 || y_start + local_ny > ny) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: strip [%d,%d) outside [0,%d)", y_start, y_start + local_ny, ny);
    if (precision != LBM_PRECISION_F64 && precision != LBM_PRECISION_F32) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: bad precision %d", precision);
    if ((arith != 0 && arith != 1) || (periodic_y != 0 && periodic_y != 1)) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: arith and periodic_y are 0 or 1");
    const RegionKind* kind = deep_kind(deep);
    if (!kind) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: deep %d is no register shape", deep);
    const RowsWaves rw = col_rw(*kind, precision == LBM_PRECISION_F32 ? 4 : 8, arith != 0);
    if (!rw.rows) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: deep %d (%s regions) is not built for this precision and arithmetic", deep, kind->name);
    if (!col_depth(*kind, depth)) return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: %s regions offer no launch of %d iterations", kind->name, depth);
    if (y_cnt <= 0) { y_lo = 0; y_cnt = local_ny; }
    const int HW = depth - 1, OW = col_tile_w(depth), OH = col_tile_h(depth, rw);
    const int nbx = (nx + OW - 1) / OW, nby = (y_cnt + OH - 1) / OH;
    if (bx < 0 || bx >= nbx || by < 0 || by >= nby || wave < 0 || wave >= rw.waves)
        return fail(LBM_ERR_ARG, "lbm_debug_wave_plain: tile (%d, %d) of %d x %d, wave %d of %d", bx, by, nbx, nby, wave, rw.waves);
    lbm_ctx* c = choreo_fake_ctx(nx, ny, y_start, local_ny, precision, 0);      // (row-interleaved, as every deep plan is)
    c->periodic_y = periodic_y;
    if (cylinder3) { c->cyl_x = (int)(cylinder3[0] * nx); c->cyl_y = (int)(cylinder3[1] * ny); c->cyl_r = (int)(cylinder3[2] * ny); }
    KArgs<double> a{};
    a.nx = nx; a.ny_loc = local_ny; a.ny_glob = rows_glob(c); a.y_start = row_start(c);
    a.cyl_x = c->cyl_x; a.cyl_y = c->cyl_y; a.cyl_r2 = (double)(c->cyl_r * c->cyl_r);
    a.y_lo = y_lo; a.y_cnt = y_cnt;
    HostMask h;
    if (periodic_y) {       // (prepare_periodic: the wrapped window of the mask or of the disc)
        const double r2 = a.cyl_r2;
        h = pack_mask_periodic([&](int x, int, int y) {
            if (mask) return mask[(size_t)y * nx + x] != 0;
            const double dx = x - c->cyl_x, dy = y - c->cyl_y;
            return dx * dx + dy * dy <= r2;
        }, nx, ny, y_start, local_ny, PERIODIC_PAD);
    } else if (mask) h = pack_mask(mask, nx, ny, y_start, local_ny);
    if (periodic_y || mask) a.mv = h.view();
    const bool small = buffer_small(c);
    delete c;
    const int y_end = y_lo + y_cnt, Xo = bx * OW, Yo = y_lo + by * OH;               // (band_origin, first range)
    const bool near = tile_near_solid(a, Xo, Yo, OW, OH, HW);
    if (dims4) {
        const int yg0 = a.y_start + Yo;
        const bool lean = !near && Xo >= HW + 1 && Xo + OW + HW <= nx - 1 && yg0 >= HW + 1 && yg0 + OH + HW <= a.ny_glob - 1 && Yo + OH <= y_end && small;   // (TileFrame::lean)
        dims4[0] = rw.rows; dims4[1] = rw.waves; dims4[2] = lean ? 1 : 0; dims4[3] = near ? 1 : 0;
    }
    return wave_plain(nx, a.ny_glob, a.y_start, Xo, Yo, y_end, OW, OH, HW, near, small, wave * rw.rows, rw.rows) ? 1 : 0;
}

/* TEST HOOK (no device needed): what lbm_set_body_labels uploads for the strip [y_start, y_start + local_ny) (csrc/lbm_geom.hpp pack_bodies). */
int lbm_debug_body_chunks(const unsigned char* labels, int nx, int ny, int y_start, int local_ny, int* boxes4, int boxes_cap,
                          long* chunks3, int chunks_cap, int* nchunks_out) {
    if (!labels || nx < 1 || ny < 1 || y_start < 0 || local_ny < 1 || y_start + local_ny > ny) return fail(LBM_ERR_ARG, "bad argument");
    const HostBodies h = pack_bodies(labels, nx, ny, y_start, local_ny);
    if (nchunks_out) *nchunks_out = (int)h.chunks.size();
    if (boxes4) {
        if (boxes_cap < h.B) return fail(LBM_ERR_ARG, "boxes: %d entries needed", h.B);
        if (h.B) memcpy(boxes4, h.box.data(), h.box.size() * sizeof(int));
    }
    if (chunks3) {
        if (chunks_cap < (int)h.chunks.size()) return fail(LBM_ERR_ARG, "chunks: %zu entries needed", h.chunks.size());
        for (size_t k = 0; k < h.chunks.size(); ++k) { chunks3[3 * k] = h.chunks[k].body; chunks3[3 * k + 1] = h.chunks[k].first; chunks3[3 * k + 2] = h.chunks[k].cells; }
    }
    return h.B;
}

/* TEST HOOK (no device needed): the candidates lbm_initialise would time for a whole-domain context of this grid, one per line:
 * "name|lbm_set_option pairs|dominant kernel|iterations per launch". arith: 0 / 1, 2 / 3 for a Smagorinsky (LES) context, 4 / 5 for a TRT one,
 * 8 / 9 for one with a driving force (lbm_set_forcing), 16 / 17 for an MRT one (lbm_set_mrt), 32 / 33 for one with an outlet sponge
 * (lbm_set_sponge). */
int lbm_debug_plan_candidates(int nx, int ny, int precision, int arith, int num_cus, char* out, int cap) {
    if (!out || cap < 1 || nx < 1 || ny < 1) return fail(LBM_ERR_ARG, "bad argument");
    PlanQuery q;
    q.nx = nx; q.nyl = ny; q.ny_glob = ny; q.esize = precision == LBM_PRECISION_F32 ? 4 : 8; q.num_cus = num_cus > 0 ? num_cus : 256;
    q.no_tall = !collision_model(arith).tall;
    q.park = (arith & 1) && collision_model(arith).park;
    const Plan none{};
    std::string text;
    for (const Plan& pl : plan_candidates(q, none)) {
        const int fuse = pl.fuse > 0 ? pl.fuse : 1;
        text += pl.name + "|" + plan_option_string(pl.layout, pl.nt, pl.alternate, pl.ty, pl.xcd, fuse, pl.deep, pl.ntl) + "|" +
                plan_kernel_name(fuse, pl.deep, pl.ty ? pl.ty : 8, pl.nt, arith, q.esize) + "|" + std::to_string(pl.deep ? deep_depth(pl.deep) : fuse) + "\n";
    }
    if ((int)text.size() + 1 > cap) return fail(LBM_ERR_ARG, "buffer too small (%zu bytes needed)", text.size() + 1);
    memcpy(out, text.c_str(), text.size() + 1);
    return LBM_OK;
}

/* TEST HOOK (no device needed): the deep launch shapes (deep_shapes and region_kinds, lbm_plan.hpp), one line per id, precision and
 * arithmetic mode that exists: see include/lbm_hip.h. */
int lbm_debug_deep_shapes(char* out, int cap) {
    if (!out || cap < 1) return fail(LBM_ERR_ARG, "bad argument");
    std::string text;
    char b[160];
    for (const DeepShape& s : deep_shapes)
        for (int esize : {8, 4})
            for (int contracted : {0, 1}) {
                const RegionKind* k = deep_kind(s.id);
                const RowsWaves rw = k ? col_rw(*k, esize, contracted) : RowsWaves{1, s.tile_w * s.tile_h / 64};     // (an LDS tile: a cell per thread)
                if (!rw.rows) continue;
                snprintf(b, sizeof(b), "%d|%s|%s|%s|%d|%d|%d|%d|%d|", s.id, esize == 8 ? "f64" : "f32", contracted ? "contracted" : "strict", k ? "registers" : "lds",
                         s.depth, k ? 64 : s.tile_w, k ? rw.rows * rw.waves : s.tile_h, rw.rows, rw.waves);
                text += b;
                if (!k) text += std::to_string(s.depth);
                else for (const ColDepth& d : k->depths)
                    text += (&d == k->depths ? "" : " ") + std::to_string(d.depth) + (d.nt ? ":nt+plain" : ":plain") + (d.no_face ? ":no-face" : "");
                const bool one = k && !k->rw[esize != 4][0].rows && !k->rw[esize != 4][1].rows;       // (the other precision has none)
                text += std::string("|") + (one ? (esize == 8 ? "fp64 only" : "fp32 only") : "") + (k && k->only ? std::string(", ") + k->only : "") +
                        (k && k->needs ? (k->needs == &CollisionModel::tall ? ", model flag tall" : ", model flag park") : "") + "\n";
            }
    if ((int)text.size() + 1 > cap) return fail(LBM_ERR_ARG, "buffer too small (%zu bytes needed)", text.size() + 1);
    memcpy(out, text.c_str(), text.size() + 1);
    return LBM_OK;
}

/* TEST HOOK (no device needed): wall_rule (lbm_kernels.hpp), the function the kernels call, on one cell in the element type of `precision`. */
int lbm_debug_wall_rule(int side, int kind, double velocity, int precision, const double* f_in9, double* f_out9) {
    if (!f_in9 || !f_out9) return fail(LBM_ERR_ARG, "lbm_debug_wall_rule: null pointer");
    if (precision != LBM_PRECISION_F64 && precision != LBM_PRECISION_F32) return fail(LBM_ERR_ARG, "lbm_debug_wall_rule: precision = %d", precision);
    if (int rc = check_wall("lbm_debug_wall_rule", side, kind, velocity)) return rc;
    if (precision == LBM_PRECISION_F32) debug_wall_rule<float>(side, kind, velocity, f_in9, f_out9);
    else debug_wall_rule<double>(side, kind, velocity, f_in9, f_out9);
    return LBM_OK;
}

/* TEST HOOK (no device needed): port_rule (lbm_kernels.hpp), the function the kernels call, on one cell in the element type of `precision`. */
int lbm_debug_port_rule(int side, int kind, double value, double u_in, int precision, const double* f_in9, double* f_out9, double* rho_out, double* u_out) {
    if (!f_in9 || !f_out9) return fail(LBM_ERR_ARG, "lbm_debug_port_rule: null pointer");
    if (precision != LBM_PRECISION_F64 && precision != LBM_PRECISION_F32) return fail(LBM_ERR_ARG, "lbm_debug_port_rule: precision = %d", precision);
    if (int rc = check_port("lbm_debug_port_rule", side, kind, value)) return rc;
    if (!std::isfinite(u_in) || std::fabs(u_in) >= 1.0) return fail(LBM_ERR_ARG, "lbm_debug_port_rule: u_in = %g (finite values of magnitude below 1 only)", u_in);
    if (precision == LBM_PRECISION_F32) debug_port_rule<float>(side, kind, value, u_in, f_in9, f_out9, rho_out, u_out);
    else debug_port_rule<double>(side, kind, value, u_in, f_in9, f_out9, rho_out, u_out);
    return LBM_OK;
}

/* TEST HOOK (no device needed): the factor (double)(T)s(t) of each of nt iterations, through inlet_sched_index (lbm_kernels.hpp), the function
 * the kernels and the snapshot call. */
int lbm_debug_inlet_scale(const double* s, int n, int mode, int precision, const int* t, int nt, double* out) {
    if (!t || !out || nt < 0) return fail(LBM_ERR_ARG, "lbm_debug_inlet_scale: null pointer or nt < 0");
    if (precision != LBM_PRECISION_F64 && precision != LBM_PRECISION_F32) return fail(LBM_ERR_ARG, "lbm_debug_inlet_scale: precision = %d", precision);
    if (int rc = check_schedule("lbm_debug_inlet_scale", s, n, mode)) return rc;
    if (n == 0) return fail(LBM_ERR_ARG, "lbm_debug_inlet_scale: n = 0 (an empty table has no factor)");
    for (int i = 0; i < nt; ++i) {
        if (t[i] < 0) return fail(LBM_ERR_ARG, "lbm_debug_inlet_scale: t[%d] = %d (iterations count from 0)", i, t[i]);
        const double v = s[inlet_sched_index(t[i], n, mode)];
        out[i] = precision == LBM_PRECISION_F32 ? (double)(float)v : v;
    }
    return LBM_OK;
}

/* TEST HOOK (device 0): strict_div2 (the shared-reciprocal form of the collision's two divisions by rho, lbm_kernels.hpp) beside
 * the compiler's IEEE divisions on the same operands: q1,q2 = strict_div2(a1,a2,b); r1,r2 = a1/b, a2/b. Host arrays of n doubles. */
int lbm_debug_strict_div2(const double* a1, const double* a2, const double* b, int n, double* q1, double* q2, double* r1, double* r2) {
    if (!a1 || !a2 || !b || !q1 || !q2 || !r1 || !r2 || n < 1) return fail(LBM_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(0));
    double* d = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    HIPCHK(hipMalloc(&d, 7 * nb));
    int rc = LBM_OK;
    auto chk = [&](hipError_t e) { if (e != hipSuccess && rc == LBM_OK) rc = fail(LBM_ERR_HIP, "%s", hipGetErrorString(e)); };
    chk(hipMemcpy(d, a1, nb, hipMemcpyHostToDevice)); chk(hipMemcpy(d + n, a2, nb, hipMemcpyHostToDevice)); chk(hipMemcpy(d + 2 * (size_t)n, b, nb, hipMemcpyHostToDevice));
    if (rc == LBM_OK) {
        hipLaunchKernelGGL(k_debug_strict_div2<0>, dim3((n + 255) / 256), dim3(256), 0, nullptr, d, d + n, d + 2 * (size_t)n, n, d + 3 * (size_t)n, d + 4 * (size_t)n, d + 5 * (size_t)n, d + 6 * (size_t)n);
        chk(hipGetLastError());
        chk(hipDeviceSynchronize());
        chk(hipMemcpy(q1, d + 3 * (size_t)n, nb, hipMemcpyDeviceToHost)); chk(hipMemcpy(q2, d + 4 * (size_t)n, nb, hipMemcpyDeviceToHost));
        chk(hipMemcpy(r1, d + 5 * (size_t)n, nb, hipMemcpyDeviceToHost)); chk(hipMemcpy(r2, d + 6 * (size_t)n, nb, hipMemcpyDeviceToHost));
    }
    (void)hipFree(d);
    return rc;
}

/* TEST HOOK (no device needed): the decision tune_strip_schedule takes from per-rank pins. ranks x {tune-able, overlap_pinned,
 * overlap, deep_pinned, deep_halo}; returns LBM_OK and the agreed {go, overlap_pinned, overlap, deep_pinned, deep_halo} or LBM_ERR_ARG. */
int lbm_debug_strip_pins(const int* per_rank7, int nranks, int* agreed7) {
    if (!per_rank7 || !agreed7 || nranks < 1) return fail(LBM_ERR_ARG, "null argument");
    double m[7] = {1e30, 1e30, 1e30, 1e30, 1e30, 1e30, 1e30};
    for (int r = 0; r < nranks; ++r) {
        double v[7];
        const int* q = per_rank7 + 7 * r;
        strip_pins_pack(q[0] != 0, q[1] != 0, q[2], q[3] != 0, q[4], q[5] != 0, q[6], v);
        for (int k = 0; k < 7; ++k) m[k] = std::min(m[k], v[k]);        // what allreduce_doubles(..., MIN) returns on every rank
    }
    agreed7[2] = agreed7[4] = agreed7[6] = -1;
    if (!strip_pins_agree(m, &agreed7[0], &agreed7[1], &agreed7[2], &agreed7[3], &agreed7[4], &agreed7[5], &agreed7[6]))
        return fail(LBM_ERR_ARG, "the ranks pin different strip schedules");
    return LBM_OK;
}

/* TEST HOOK (no device needed): the runs of the halo message of a face of `hr` rows (csrc/lbm_strips.inc.hpp face_runs): up to five
 * {first sub-row, sub-rows} pairs relative to the block's first sub-row; south_block: the block lies below the strip it borders. */
int lbm_debug_face_runs(int hr, int trim, int south_block, int* runs10) {
    if (!runs10 || hr < 1) return fail(LBM_ERR_ARG, "bad argument");
    const FaceRuns r = face_runs(hr, trim != 0, south_block != 0);
    for (int k = 0; k < r.n; ++k) { runs10[2 * k] = r.off[k]; runs10[2 * k + 1] = r.cnt[k]; }
    return r.n;
}

/* TEST HOOK (no device needed): one RingIndex (csrc/lbm_plan.hpp) driven through pushes (ops[k] < 0) and takes of up to ops[k]: see include/lbm_hip.h. */
int lbm_debug_ring(int capacity, const int* ops, int nops, int* out3) {
    if (capacity < 1 || nops < 0 || (nops > 0 && (!ops || !out3))) return fail(LBM_ERR_ARG, "bad argument");
    RingIndex r{capacity, 0, 0};
    for (int k = 0; k < nops; ++k) {
        int* o = out3 + 3 * k;
        if (ops[k] < 0) {
            o[0] = r.full() ? -1 : r.next(); o[1] = o[2] = -1;
            if (!r.full()) r.commit();
        } else {
            const RingIndex::Span s = r.oldest(ops[k]);
            o[0] = s.start; o[1] = s.n1; o[2] = s.n2;
            r.drop(s.n1 + s.n2);
        }
    }
    return r.count;
}

/* TEST HOOK (no device needed): the host threads of a group (GroupPool, csrc/lbm_ctx.hpp) on a dummy job of `rounds` rounds with one
 * rendezvous each. Strip `fail_strip` reports an injected error in round `fail_round`; strip `stall_strip` sleeps `stall_ms` before
 * the rendezvous of round `stall_round` (-1: nobody). The job runs `repeat` times on the same pool. Returns what the LAST run returned
 * (LBM_OK / the injected LBM_ERR_HIP / LBM_ERR_TIMEOUT / "timed out earlier"); *rendezvous_out = rendezvous strip 0 passed in the last run. */
int lbm_debug_group_pool(int n, int rounds, int fail_strip, int fail_round, int stall_strip, int stall_round, int stall_ms, long timeout_ms, int repeat,
                         int* rendezvous_out) {
    if (n < 2 || n > 64 || rounds < 1 || repeat < 1) return fail(LBM_ERR_ARG, "bad argument");
    GroupPool pool(n);
    auto passed = std::make_shared<std::atomic<int>>(0);
    int rc = LBM_OK;
    for (int rep = 0; rep < repeat; ++rep) {
        passed->store(0);
        const bool last = rep + 1 == repeat;
        rc = pool.run([=](GroupPool::State& P, int i) {
            for (int r = 0; r < rounds; ++r) {
                if (last && i == fail_strip && r == fail_round) P.report(fail(LBM_ERR_HIP, "injected fault: strip %d, round %d", i, r), g_err);
                if (last && i == stall_strip && r == stall_round) std::this_thread::sleep_for(std::chrono::milliseconds(stall_ms));
                if (P.arrive(i, r, 1)) return;
                if (i == 0) passed->fetch_add(1);
            }
        }, timeout_ms);
    }
    if (rendezvous_out) *rendezvous_out = passed->load();
    return rc;        // (~GroupPool: waits, bounded, for a straggler and joins; a thread that never comes back is detached)
}

/* TEST HOOK (no device needed): dry run of the launch choreography of a strip run and its check (csrc/lbm_choreo.inc.hpp). */
int lbm_debug_choreography(int nx, int ny, const int* bounds2, int nstrips, int precision, int transport, const char* options,
                           const int* calls2, int ncalls, int dump, char* out, int cap) {
    if (!bounds2 || nstrips < 1 || !calls2 || ncalls < 1 || (out && cap < 1) || transport < 0 || transport > 3) return fail(LBM_ERR_ARG, "bad argument");
    if (transport >= 2 && nstrips != 1) return fail(LBM_ERR_ARG, "transports 2 (one rank of a multi-process run) and 3 (loopback) describe ONE strip");
    std::vector<lbm_ctx*> cs;
    Choreo rec;
    auto cleanup = [&]() { for (lbm_ctx* c : cs) delete c; };
    for (int k = 0; k < nstrips; ++k) {
        lbm_ctx* c = choreo_fake_ctx(nx, ny, bounds2[2 * k], bounds2[2 * k + 1], precision, k);
        cs.push_back(c);
        if (c->p.y_start < 0 || c->nyl < 1 || c->p.y_start + c->nyl > ny) { cleanup(); return fail(LBM_ERR_ARG, "strip %d outside the lattice", k); }
        for (const char* q = options ? options : ""; *q;) {        // "key=value key=value"
            while (*q == ' ') ++q;
            const char* eq = strchr(q, '=');
            if (!eq) break;
            const std::string key(q, eq);
            char* end = nullptr;
            const long v = strtol(eq + 1, &end, 10);
            const int rc = lbm_set_option(c, key.c_str(), v);
            if (rc) { cleanup(); return rc; }
            q = end;
        }
        c->layout = 1; configure_layout(c, 1);        // strips: row-interleaved
        if (c->deep) c->fuse = deep_depth(c->deep);
        if (transport == 2) {      // rank and size as the strip's faces say
            const bool s_face = c->p.y_start > 0, n_face = c->p.y_start + c->nyl < ny;
            c->comm = (ncclComm_t)(uintptr_t)0x1;
            c->nranks = 1 + (s_face ? 1 : 0) + (n_face ? 1 : 0);
            c->rank = s_face ? 1 : 0;
        } else if (transport == 3) c->loopback = 1;
        if (c->periodic_y && transport >= 2) { cleanup(); return fail(LBM_ERR_ARG, "periodic_y=1 goes with transports 0 and 1 (a ring of strips; one strip: a periodic context on its own)"); }
        if (int rc = refuse_deep(c, c->collision, c->deep, true)) { cleanup(); return rc; }       // (as lbm_initialise does)
        c->initialised = true;
        c->cur = 1;
        if (c->stats_opt >= 0) { c->stats_active = true; c->stats_from = c->stats_opt; }      // (no accumulators: nothing is launched)
        if (c->bodies_opt) { c->body_n = 1; c->body_log.ix.cap = c->log_cap; }                // (no labels and no log either)
        if (c->frames_opt > 0) { c->frames_active = true; c->frames_k = c->frames_opt; }      // (no ring: nothing is launched)
        if (c->probes_opt) { c->probes_active = true; c->probe_n = 1; }                       // (no table and no ring either)
    }
    if (transport < 2) {
        for (int k = 0; k < nstrips; ++k) {
            cs[(size_t)k]->nb_south = k > 0 ? cs[(size_t)k - 1] : nullptr;
            cs[(size_t)k]->nb_north = k + 1 < nstrips ? cs[(size_t)k + 1] : nullptr;
            if (nstrips > 1) {      // (periodic_y=1: the ring; one strip is a periodic context on its own)
                cs[(size_t)k]->ring_south = k == 0 ? cs[(size_t)nstrips - 1] : nullptr;
                cs[(size_t)k]->ring_north = k + 1 == nstrips ? cs[0] : nullptr;
            }
            if (cs[(size_t)k]->periodic_y != cs[0]->periodic_y || (cs[0]->periodic_y && cs[(size_t)k]->nyl < 2 * HR1)) { cleanup(); return fail(LBM_ERR_ARG, "periodic y: every strip alike, and at least %d rows each", 2 * HR1); }
            cs[(size_t)k]->group_transport = transport; cs[(size_t)k]->group_n = nstrips; cs[(size_t)k]->group_threads = 0;
            const int expect = k == 0 ? 0 : cs[(size_t)k - 1]->p.y_start + cs[(size_t)k - 1]->nyl;
            if (cs[(size_t)k]->p.y_start != expect || (k + 1 == nstrips && expect + cs[(size_t)k]->nyl != ny)) { cleanup(); return fail(LBM_ERR_ARG, "the strips must cover the lattice bottom to top"); }
        }
    }
    ChoreoChecker chk;
    chk.init(cs.data(), nstrips);       // (before `rec` is set: the initial state is what lbm_initialise leaves)
    for (lbm_ctx* c : cs) c->rec = &rec;
    int rc = LBM_OK;
    for (int k = 0; k < ncalls && !rc; ++k)
        rc = DISPATCH(cs[0], do_steps<double>(cs.data(), nstrips, calls2[2 * k], calls2[2 * k + 1]), do_steps<float>(cs.data(), nstrips, calls2[2 * k], calls2[2 * k + 1]));
    if (rc) { cleanup(); return rc; }
    chk.run(rec.ops);
    std::string text;
    for (const ChoreoViolation& v : chk.bad) {
        char b[96];
        if (v.kind == 0) {
            snprintf(b, sizeof(b), "RACE strip %d buffer %d row %d:\n   ", v.strip, v.buf, v.row);
            text += b + choreo_op_text(rec.ops[(size_t)v.op_a], v.op_a) + "\n   " + choreo_op_text(rec.ops[(size_t)v.op_b], v.op_b) + "\n";
        } else {
            snprintf(b, sizeof(b), "STALE strip %d buffer %d row %d holds iteration %d, wanted %d:\n   ", v.strip, v.buf, v.row, v.have == INT_MIN ? -1 : v.have, v.want);
            text += b + choreo_op_text(rec.ops[(size_t)v.op_a], v.op_a) + "\n";
        }
        if (text.size() > 6000) break;
    }
    if (dump) for (int i = 0; i < (int)rec.ops.size(); ++i) text += choreo_op_text(rec.ops[(size_t)i], i) + "\n";
    if (out) { const size_t m = std::min(text.size(), (size_t)cap - 1); memcpy(out, text.data(), m); out[m] = 0; }
    const int nbad = (int)chk.bad.size();
    cleanup();
    return nbad;
}

/* TEST HOOK (no device needed): the collision models' setters on a context no device knows: see include/lbm_hip.h. */
int lbm_debug_collision_setters(double tau, int precision, const char* options, const int* setter, const double* v1, const double* v2, int n,
                                int* rc, char* texts, int cap, double* collision3) {
    if (!setter || !v1 || !v2 || n < 0 || !rc || !texts || cap < 1 || !collision3) return fail(LBM_ERR_ARG, "lbm_debug_collision_setters: null argument");
    lbm_ctx* c = choreo_fake_ctx(64, 64, 0, 64, precision, 0);
    c->p.tau = tau;
    for (const char* q = options ? options : ""; *q;) {        // "key=value key=value"
        while (*q == ' ') ++q;
        const char* eq = strchr(q, '=');
        if (!eq) break;
        const std::string key(q, eq);
        char* end = nullptr;
        const long v = strtol(eq + 1, &end, 10);
        if (int orc = lbm_set_option(c, key.c_str(), v)) { delete c; return orc; }
        q = end;
    }
    std::string text;
    int bad = LBM_OK;
    for (int k = 0; k < n && !bad; ++k) {
        switch (setter[k]) {
            case 0: rc[k] = lbm_set_smagorinsky(c, v1[k]); break;
            case 1: rc[k] = lbm_set_trt(c, v1[k]); break;
            case 2: rc[k] = lbm_set_forcing(c, v1[k], v2[k]); break;
            case 3: rc[k] = lbm_set_mrt(c, v1[k], v2[k]); break;
            case 4: c->initialised = true; rc[k] = LBM_OK; break;
            case 5: rc[k] = refuse_deep(c, c->collision, c->deep, true); break;
            case 6: rc[k] = lbm_set_sponge(c, (int)v1[k], v2[k]); break;
            default: bad = LBM_ERR_ARG; continue;
        }
        if (rc[k]) text += lbm_last_error();
        text += "\n";
    }
    collision3[0] = c->collision;
    (void)lbm_get_mrt(c, &collision3[1], &collision3[2]);
    delete c;
    if (bad) return fail(LBM_ERR_ARG, "lbm_debug_collision_setters: setter 0..6 only");
    if ((int)text.size() + 1 > cap) return fail(LBM_ERR_ARG, "lbm_debug_collision_setters: buffer too small (%zu bytes needed)", text.size() + 1);
    memcpy(texts, text.c_str(), text.size() + 1);
    return LBM_OK;
}

/* TEST HOOK (no device needed): the launch-uniform values of one collision model as make_kargs stores them and the slot map reads them
 * back: see include/lbm_hip.h. */
int lbm_debug_collision_args(double tau, int precision, int setter, double v1, double v2, double* out, int cap) {
    if (!out || cap < 0) return fail(LBM_ERR_ARG, "lbm_debug_collision_args: null pointer or negative capacity");
    lbm_ctx* c = choreo_fake_ctx(64, 64, 0, 64, precision, 0);
    c->p.tau = tau;
    int rc = LBM_OK;
    switch (setter) {
        case -1: break;
        case 0: rc = lbm_set_smagorinsky(c, v1); break;
        case 1: rc = lbm_set_trt(c, v1); break;
        case 2: rc = lbm_set_forcing(c, v1, v2); break;
        case 3: rc = lbm_set_mrt(c, v1, v2); break;
        case 6: rc = lbm_set_sponge(c, (int)v1, v2); break;
        default: rc = fail(LBM_ERR_ARG, "lbm_debug_collision_args: setter -1, 0, 1, 2, 3 or 6 only");
    }
    auto read = [&](auto element) -> int {      // (a generic lambda: this part of the file has C linkage)
        using T = decltype(element);
        const KArgs<T> a = make_kargs<T>(c, 0, 1, 0);
        std::vector<double> v;
        switch (c->collision) {
            case AR_STRICT: { const BgkK<T> k = bgk_k(a); v = {(double)k.wp}; break; }
            case AR_STRICT_LES: { const LesK<T> k = les_k(a); v = {(double)k.tau, (double)k.tau2, (double)k.c}; break; }
            case AR_STRICT_TRT: { const TrtK<T> k = trt_k(a); v = {(double)k.wp, (double)k.wm, (double)k.wa, (double)k.wb}; break; }
            case AR_STRICT_FORCED: { const ForcedK<T> k = forced_k(a); v = {(double)k.wp, (double)k.gx, (double)k.gy, (double)k.hx, (double)k.hy}; break; }
            case AR_STRICT_MRT: { const MrtK<T> k = mrt_k(a); v = {(double)k.wp, (double)k.wm, (double)k.wa, (double)k.wb, (double)k.sb, (double)k.kb}; break; }
            default: break;      // the outlet sponge: nothing launch-uniform beyond its table
        }
        const int named = (int)v.size();
        for (T raw : shared_collision_slots(a)) v.push_back((double)raw);
        if ((int)v.size() > cap) return fail(LBM_ERR_ARG, "lbm_debug_collision_args: %zu values, room for %d", v.size(), cap);
        std::copy(v.begin(), v.end(), out);
        return named;
    };
    if (rc == LBM_OK) rc = precision == LBM_PRECISION_F32 ? read(float{}) : read(double{});
    delete c;
    return rc;
}

/* TEST HOOK (no device needed): lbm_set_sponge on a context no device knows, and the rate of every column: see include/lbm_hip.h. */
int lbm_debug_sponge_rates(int nx, double tau, int precision, int width, double tau_end, double* pair2, double* rates) {
    if (!pair2 || !rates || nx < 1) return fail(LBM_ERR_ARG, "lbm_debug_sponge_rates: null pointer or nx < 1");
    lbm_ctx* c = choreo_fake_ctx(nx, 64, 0, 64, precision, 0);
    c->p.tau = tau;
    const int rc = lbm_set_sponge(c, width, tau_end);
    const std::string text = rc ? lbm_last_error() : "";
    int w = 0;
    (void)lbm_get_sponge(c, &w, &pair2[1]);
    pair2[0] = w;
    for (int x = 0; x < nx; ++x) (void)lbm_get_sponge_rate(c, x, &rates[x]);
    delete c;
    return rc ? fail(rc, "%s", text.c_str()) : LBM_OK;
}

/* TEST HOOK (no device needed): every rank of a multi-process strip run issues its launch groups DRY (as lbm_debug_choreography does for one
 * rank) and the transcripts of exchange_rccl's posting loops are paired: see include/lbm_hip.h. */
int lbm_debug_p2p_matching(int nx, int ny, const int* bounds2, int nranks, int precision, const char* options, const char* options_rank1,
                           const int* calls2, int ncalls, char* out, int cap) {
    if (!bounds2 || nranks < 2 || !calls2 || ncalls < 1 || (out && cap < 1)) return fail(LBM_ERR_ARG, "bad argument");
    std::vector<lbm_ctx*> cs;
    std::vector<Choreo> rec((size_t)nranks);
    auto cleanup = [&]() { for (lbm_ctx* c : cs) delete c; };
    auto apply = [&](lbm_ctx* c, const char* opts) -> int {
        for (const char* q = opts ? opts : ""; *q;) {
            while (*q == ' ') ++q;
            const char* eq = strchr(q, '=');
            if (!eq) break;
            const std::string key(q, eq);
            char* end = nullptr;
            const long v = strtol(eq + 1, &end, 10);
            const int rc = lbm_set_option(c, key.c_str(), v);
            if (rc) return rc;
            q = end;
        }
        return LBM_OK;
    };
    for (int k = 0; k < nranks; ++k) {
        lbm_ctx* c = choreo_fake_ctx(nx, ny, bounds2[2 * k], bounds2[2 * k + 1], precision, 0);
        cs.push_back(c);
        const int expect = k == 0 ? 0 : cs[(size_t)k - 1]->p.y_start + cs[(size_t)k - 1]->nyl;
        if (c->nyl < 1 || c->p.y_start != expect || (k + 1 == nranks && expect + c->nyl != ny)) { cleanup(); return fail(LBM_ERR_ARG, "the strips must cover the lattice bottom to top"); }
        int rc = apply(c, options);
        if (!rc && k == 1) rc = apply(c, options_rank1);
        if (!rc && c->periodic_y) rc = fail(LBM_ERR_ARG, "lbm_debug_p2p_matching: periodic_y=1 (rings of processes are not built: lbm_initialise refuses them)");
        if (rc) { cleanup(); return rc; }
        c->layout = 1; configure_layout(c, 1);
        if (c->deep) c->fuse = deep_depth(c->deep);
        c->comm = (ncclComm_t)(uintptr_t)0x1; c->rank = k; c->nranks = nranks;
        c->initialised = true; c->cur = 1;
        c->rec = &rec[(size_t)k];
        for (int q = 0; q < ncalls && !rc; ++q)
            rc = DISPATCH(c, do_steps<double>(&c, 1, calls2[2 * q], calls2[2 * q + 1]), do_steps<float>(&c, 1, calls2[2 * q], calls2[2 * q + 1]));
        if (rc) { cleanup(); return rc; }
    }
    std::string text;
    int bad = 0;
    auto pick = [&](int r, int kind, int peer) { std::vector<ChoreoP2P> v; for (const ChoreoP2P& p : rec[(size_t)r].p2p) if (p.kind == kind && p.peer == peer) v.push_back(p); return v; };
    auto groups = [&](int r) { int n = 0; for (const ChoreoP2P& p : rec[(size_t)r].p2p) n += p.kind == 2; return n; };
    auto pair_up = [&](int from, int to, long from_block, long to_block, const char* what) {
        const std::vector<ChoreoP2P> S = pick(from, 0, to), R = pick(to, 1, from);
        char b[256];
        if (S.size() != R.size()) { ++bad; snprintf(b, sizeof(b), "%s: rank %d posts %zu sends to rank %d, which posts %zu receives from it\n", what, from, S.size(), to, R.size()); text += b; return; }
        for (size_t k = 0; k < S.size(); ++k)
            if (S[k].cnt != R[k].cnt || S[k].off - from_block != R[k].off - to_block) {
                ++bad;
                if (text.size() < 3000) { snprintf(b, sizeof(b), "%s: message %zu: rank %d sends %ld elements from block offset %ld, rank %d receives %ld at block offset %ld\n", what, k, from,
                                                   S[k].cnt, S[k].off - from_block, to, R[k].cnt, R[k].off - to_block); text += b; }
            }
    };
    for (int r = 0; r + 1 < nranks; ++r) {
        const FaceSpans lo = face_spans(cs[(size_t)r]), hi = face_spans(cs[(size_t)r + 1]);
        pair_up(r, r + 1, lo.top_rows, hi.ghost_s, "northbound");
        pair_up(r + 1, r, hi.bot_rows, lo.ghost_n, "southbound");
        if (groups(r) != groups(r + 1)) { ++bad; char b[160]; snprintf(b, sizeof(b), "ranks %d and %d issue %d and %d exchanges\n", r, r + 1, groups(r), groups(r + 1)); text += b; }
    }
    {
        char b[160];
        snprintf(b, sizeof(b), "%d exchanges per rank, %zu messages posted by rank 0\n", groups(0), rec[0].p2p.size() - (size_t)groups(0));
        text += b;
    }
    if (out) { const size_t m = std::min(text.size(), (size_t)cap - 1); memcpy(out, text.data(), m); out[m] = 0; }
    cleanup();
    return bad;
}

const char* lbm_plan(const lbm_ctx* c) { return c ? c->plan_desc : ""; }
const char* lbm_plan_options(const lbm_ctx* c) { return c ? c->plan_opts : ""; }

#ifndef LBM_BUILD_ID_STR
#define LBM_BUILD_ID_STR "unversioned-----"
#endif
const char* lbm_build_id(void) {
    static const char tag[] = "LBM_BUILD_ID=" LBM_BUILD_ID_STR;   // the marker build.py looks for in the file
    return tag + 13;
}

}  // extern "C"

#include "lbm_group.inc.hpp"
