/* include/lbm_hip.h — C-ABI of the MI355X-native D2Q9-BGK timestep (liblbm_hip.so).
 *
 * The reference (LGMOak/HighPerformanceComputing-LatticeBoltzmannMethod) has no FFI/plugin seam: it is a
 * header-only C++ class library driven by src/main.cpp:11-20. The seam below is therefore the set of calls
 * the reference's own classes make on the hot path, one entry point per reference member, so that
 * LBM::Solver / LBM::Grid / LBM::IOManager can be re-hosted on it (see INTEGRATION.md and the C++ mirror in
 * highperformancecomputing-latticeboltzmannmethod_amd/host/). Plain C types only; all output buffers are
 * caller-owned host memory; all device memory is owned by the context; no exceptions cross the boundary.
 *
 * Return convention: 0 = ok; LBM_ERR_* (<0) = failure, text via lbm_last_error(). There is NO CPU fallback:
 * without a usable HIP device every entry point that touches state fails with LBM_ERR_HIP.
 *
 * Time convention: a context has completed `steps_done` loop bodies of Solver::run (LBMSolver.h:48-76).
 * The device holds the post-collision populations of loop body t = steps_done (the reference's f_next right
 * after collision_step() of iteration t) and those of iteration t-1, so
 *   lbm_get_forces          == IOManager::record_forces(t = steps_done, ...)      (LBMIO.h:114-168)
 *   lbm_get_macros          == rho/ux/uy as left by iteration steps_done-1         
 *   lbm_get_populations     == f_current / f_next as left by iteration steps_done-1
 */
#ifndef LBM_HIP_H
#define LBM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_OK            0
#define LBM_ERR_ARG      -1   /* bad argument / bad state */
#define LBM_ERR_HIP      -2   /* HIP runtime error or no device */
#define LBM_ERR_COMM     -3   /* RCCL error / communicator not initialised */
#define LBM_ERR_ALLOC    -4
#define LBM_ERR_TIMEOUT  -5   /* a host-side wait of the library ran into its bound (option "wait_timeout_ms", LBM_WAIT_TIMEOUT_MS): the
                               * text names who was waited for and where; a group that timed out is unusable, destroy it */

#define LBM_PRECISION_F64 0
#define LBM_PRECISION_F32 1   /* build-only variant; the reference has no fp32 path */

/* Physics: field-for-field LBM::SimulationParams (LBMConfig.h:36-51) minus the run-control fields, which
 * stay with the host-side Solver. Strip: the row strip [y_start, y_start+local_ny) of the global ny rows this
 * context owns (replaces Grid::initialise_2d_topology, LBMGrid.h:347-364; whole domain: y_start=0,
 * local_ny=ny). */
typedef struct lbm_params {
    double tau;              /* LBMConfig.h:37 */
    double inlet_velocity;   /* LBMConfig.h:38 */
    int    nx, ny;           /* LBMConfig.h:39-40, global interior size */
    double cylinder_x;       /* LBMConfig.h:46, fraction of nx */
    double cylinder_y;       /* LBMConfig.h:47, fraction of ny */
    double cylinder_radius;  /* LBMConfig.h:48, fraction of ny */
    int    y_start;          /* first global row of this strip */
    int    local_ny;         /* rows in this strip (0 => ny - y_start) */
    int    precision;        /* LBM_PRECISION_* */
    int    force_log_capacity; /* rows of the device-resident force log (0 => 4096) */
} lbm_params;

typedef struct lbm_ctx lbm_ctx;

typedef struct lbm_force_row { int timestep; double fx, fy; } lbm_force_row;
typedef struct lbm_body_force_row { int timestep; int body; double fx, fy; } lbm_body_force_row;   /* lbm_drain_body_force_log */

const char* lbm_last_error(void);
int  lbm_device_count(void);

/* Grid::Grid (LBMGrid.h:57-90): creates the context (streams, logs); the two SoA population buffers are allocated by
 * lbm_initialise, whose measured plan decides their layout. */
int  lbm_create(const lbm_params* p, int device, lbm_ctx** out);
void lbm_destroy(lbm_ctx* c);

/* Grid::setup_geometry + Grid::initialise (LBMGrid.h:152-246) followed by collision_step() of iteration 0
 * (LBMSolver.h:84-126). *solid_count_out (nullable) = solid cells in this strip (LBMGrid.h:158-175). */
int  lbm_initialise(lbm_ctx* c, int* solid_count_out);

/* `nsteps` loop bodies of Solver::run (LBMSolver.h:49-60): exchange + stream + BCs + stability of iteration
 * t, fused with collision_step() of iteration t+1; up to six (eight on grids of a single round of blocks) consecutive
 * iterations share one kernel launch, as many as the measured plan fuses
 * (intermediate states stay in LDS; results are bit-identical to one launch per iteration). Asynchronous on the
 * context's streams. If output_frequency > 0, record_forces is evaluated on-device for every
 * t % output_frequency == 0 inside the range (LBMSolver.h:52-54) and appended to the force log. The last iteration
 * of a call is always a launch of its own, so that the snapshots below refer to iteration steps_done-1.
 * With output_frequency == 0 no forces are evaluated and, with statistics begun (lbm_stats_begin), nothing is sampled. With a
 * communicator attached (lbm_comm_init) the strip's six edge rows per face are exchanged once per launch of five / six
 * iterations (strips of 64 rows or more) or once per two launches of up to three (replaces
 * Grid::exchange_ghost_cells, LBMGrid.h:249-283). */
int  lbm_step(lbm_ctx* c, int nsteps, int output_frequency);

/* Waits for everything queued on the context's two streams. Default: the blocking hipStreamSynchronize (the fastest way to wait; a
 * watchdog thread prints one "lbm_hip: STALL: ..." line on stderr — strip, stream, iteration — if it outlives LBM_WAIT_TIMEOUT_MS, five
 * minutes by default). With the option "wait_timeout_ms" set: a bounded poll that returns LBM_ERR_TIMEOUT instead of blocking on. The
 * reference's counterpart is the implicit completion of every loop body (it is synchronous, LBMSolver.h:48-76). */
int  lbm_sync(lbm_ctx* c);
int  lbm_steps_done(const lbm_ctx* c);

/* Grid::check_stability (LBMGrid.h:285-317), evaluated inside every step kernel; returns the first
 * iteration t whose post-BC populations were non-finite or outside [-1e5, 1e5] (the t the reference prints at
 * LBMSolver.h:62), or -1. Synchronises. */
int  lbm_first_unstable_step(lbm_ctx* c, int* t_out);

/* IOManager::record_forces (LBMIO.h:133-168) for t = steps_done: this strip's partial sums. Synchronises. */
int  lbm_get_forces(lbm_ctx* c, double* fx, double* fy);
/* Rows appended by lbm_step (this strip's partial sums), oldest first: all of them are copied and leave the log, and their number is
 * returned — or, where max_rows is fewer, LBM_ERR_ARG "force log holds %d rows, buffer takes %d" and the log stays. Synchronises. */
int  lbm_drain_force_log(lbm_ctx* c, lbm_force_row* rows, int max_rows);

/* ---- forces per obstacle body (no reference counterpart: the reference has one disc and one total, LBMIO.h:133-168; what this replaces
 * is a caller's lbm_get_populations — 9 (nx+2)(local_ny+2) doubles over the bus and a synchronisation per sample — and link sums on the
 * host) ----
 * lbm_set_body_labels sets the geometry exactly as lbm_set_solid_mask does with the same bytes (nonzero = solid: solid count,
 * lbm_get_solid, macros, total force and the checkpoint digest of the solid set are those of the mask) and KEEPS the bytes as labels:
 * 0 = fluid, k in 1..255 = a solid cell of body k. The body count B is the largest label present; a label in 1..B that no cell carries
 * is a body whose force is zero. The force on body k at iteration t is the part of lbm_get_forces' sum whose links END in body k: every
 * fluid cell x of this strip's rows, every direction i whose neighbour x + c_i lies in the domain and carries label k, sum 2 c_i f_i(x)
 * on the post-collision populations. A link belongs to the body of its solid end, so bodies that touch are told apart; a strip reports
 * the partial sums over the fluid cells of its own rows (strips add up; a strip that holds no cell next to a body reports zeros for it).
 * The partition of the work and the order of every sum depend on the labels and the strip alone: plans, layouts and repetitions give the
 * same bits, and where 1 is the only label the row of body 1 equals the total of lbm_get_forces / the force log bit for bit.
 * Device memory: one byte per cell of the strip's rows + one ghost row per face, read by the per-body force kernel only (the step
 * kernels keep the packed mask); the log takes 24 B x B x force_log_capacity.
 * Call after lbm_create and before lbm_initialise; every strip of a run is given the same global [ny][nx] array. A later
 * lbm_set_solid_mask clears the labels; a later lbm_set_body_labels replaces mask and labels. Labels change reporting only: checkpoints
 * are byte for byte those of a context given the same solid set as a mask, and load into either.
 * LBM_ERR_ARG: null pointer, nx / ny other than the domain's, or an initialised context (the errors of lbm_set_solid_mask). */
int  lbm_set_body_labels(lbm_ctx* c, const unsigned char* labels, int nx, int ny);
/* B of lbm_set_body_labels; 0 without labels (no reference counterpart). */
int  lbm_body_count(const lbm_ctx* c);
/* The per-body forces for t = steps_done, like lbm_get_forces: fxy = [B][2] (fx, fy of body 1 first), this strip's partial sums.
 * Synchronises. LBM_ERR_ARG without labels (no reference counterpart). */
int  lbm_get_body_forces(lbm_ctx* c, double* fxy);
/* With labels set, lbm_step / lbm_group_step append one SAMPLE of B rows (body 1..B) at exactly the iterations at which they append a
 * force-log row, issued directly behind the force kernel on the same stream without a synchronisation. The log holds
 * force_log_capacity samples (lbm_step fails when it is full: drain it). A drain copies whole samples only, oldest first — as many as
 * fit into max_rows rows (none if max_rows < B) — removes them from the log and returns the number of ROWS copied; 0 without labels.
 * Synchronises (no reference counterpart). */
int  lbm_drain_body_force_log(lbm_ctx* c, lbm_body_force_row* rows, int max_rows);

/* rho/ux/uy of this strip, row-major [local_ny][nx] (LBMGrid.h:109-111; the layout gathered at
 * LBMSolver.h:340-357). Any pointer may be NULL. Synchronises. */
int  lbm_get_macros(lbm_ctx* c, double* rho, double* ux, double* uy);
/* Grid::max_velocity (LBMGrid.h:319-344) before the cross-rank MAX and sqrt: max(ux^2+uy^2) of this strip. */
int  lbm_max_velocity_sq(lbm_ctx* c, double* out);

/* ---- time-averaged flow statistics (no reference counterpart: the reference writes instantaneous fields only, LBMIO.h:62-111; what this
 * replaces is a caller's loop of lbm_step(c, k, 0) + lbm_get_macros + host sums, one launch boundary, one synchronisation and
 * 3 nx local_ny doubles over the bus per sample) ----
 * Six running sums per cell, always in double (fp32 contexts too), in this order: sum rho, sum ux, sum uy, sum ux*ux, sum uy*uy,
 * sum ux*uy. With statistics active, lbm_step / lbm_group_step add one SAMPLE at every iteration t of a call at which they evaluate the
 * forces (output_frequency > 0 and t % output_frequency == 0) and t >= from_step, on the device, without a synchronisation. The sample
 * of iteration t is, cell for cell and bit for bit, the (rho, ux, uy) lbm_get_macros returns on a context with steps_done == t + 1
 * (moments of the post-collision populations of iteration t; inlet / outlet columns by pull + wall + Zou-He; solid cells (1, 0, 0)).
 * Every sum is S = S + v in sample order and every product is rounded to double before it is added, so the sums equal a host loop over
 * the snapshots exactly; means and Reynolds stresses (<u'u'> = S_uu / n - (S_u / n)^2, ...) are formed by the caller from the sums and
 * the sample count, which lets strips and restarted runs be combined without loss.
 * lbm_stats_begin: on an initialised context; allocates the accumulators on first use (48 B per cell, freed by lbm_destroy), zeroes the
 * sums and the sample count and activates sampling from iteration from_step on; calling it again resets. LBM_ERR_ARG: null or
 * uninitialised context, from_step < 0; LBM_ERR_ALLOC: no device memory for the accumulators. (lbm_set_option "stats" N: the same.) */
int  lbm_stats_begin(lbm_ctx* c, int from_step);
/* Stops sampling and keeps the sums (lbm_get_stat_sums still returns them). */
int  lbm_stats_end(lbm_ctx* c);
/* Samples accumulated so far (in a group: the same on every member). */
int  lbm_stats_samples(const lbm_ctx* c);
/* The six sums of this strip, [6][local_ny][nx] in the order above, rows as in lbm_get_macros. Synchronises. LBM_ERR_ARG if statistics
 * were never begun on this context. */
int  lbm_get_stat_sums(lbm_ctx* c, double* sums6);
/* Uploads sums ([6][local_ny][nx]) and a sample count the caller saved; begins first where statistics were never begun (from_step 0)
 * and otherwise leaves from_step as it was; sampling is active afterwards. Checkpoints do NOT carry statistics: the bytes of the
 * LBMCKPT1/2/3 files are unchanged and lbm_load_state leaves the accumulators alone; a run resumed with lbm_load_state continues its
 * averages through this call. */
int  lbm_stats_restore(lbm_ctx* c, const double* sums6, int samples);

/* ---- coarsened flow frames with vorticity (no reference counterpart: the reference gathers full-resolution fields for every VTK frame,
 * LBMSolver.h:340-357, and scripts/visualise_results.py recomputes the vorticity on the host from velocity_field.csv; what this replaces
 * is a caller's lbm_step(c, n, 0) + lbm_get_macros per picture: a synchronisation and 3 nx local_ny doubles over the bus each time) ----
 * The FRAME of iteration t with stride k is four planes [local_ny / k][nx / k] of float, in the order rho, ux, uy, vorticity. Fine
 * fields: (rho, ux, uy) are, cell for cell, what lbm_get_macros returns on a context with steps_done == t + 1 (the statistics sample's
 * definition; fp32 contexts widen to double first). Vorticity w = d uy / dx - d ux / dy on the fine grid in double: the central
 * difference 0.5 * (v[x+1] - v[x-1]) inside, the one-sided v[1] - v[0] and v[n-1] - v[n-2] on the four edges of the DOMAIN (global
 * columns 0, nx - 1 and rows 0, ny - 1; a strip face is interior: the neighbour's row comes from the ghost rows); solid cells enter with
 * their (0, 0) and get their w by the same formula. Each coarse value is the mean over its k x k fine cells: summed in double (per fine
 * column bottom to top, then the k columns left to right), divided by k * k, rounded once to float. The order depends on k alone: every
 * plan, layout, arithmetic mode and strip decomposition gives the same bits for the same macros. k = 1: the fine grid plus w.
 * With frames active lbm_step / lbm_group_step append one frame to a device ring at exactly the iterations at which they append a
 * force-log row (output_frequency > 0 and t % output_frequency == 0), directly behind the force kernel, without a synchronisation;
 * with the ring full they fail like the force logs (LBM_ERR_ARG, "frame ring full ...: drain it"). Frames change reporting only:
 * populations, force logs, statistics, checkpoints (which do not carry frames) and lbm_kernel_name are those of a run without.
 * lbm_frames_begin: on an initialised context; 1 <= k <= 64, and nx, the strip's y_start and its local_ny multiples of k; capacity >= 1
 * frames. Allocates the ring (4 (nx / k) (local_ny / k) floats per frame; freed by lbm_destroy); calling it again — or lbm_initialise —
 * empties the ring. LBM_ERR_ARG (the text names the offending quantity) otherwise; LBM_ERR_ALLOC: no device memory for the ring.
 * (lbm_set_option "frames" K: the same with LBM_FRAMES_DEFAULT_CAPACITY frames.) */
#define LBM_FRAMES_DEFAULT_CAPACITY 8
int  lbm_frames_begin(lbm_ctx* c, int k, int capacity);
/* Stops sampling and keeps the undrained frames. */
int  lbm_frames_end(lbm_ctx* c);
/* Frames in the ring that have not been drained (in a group: the same on every member). */
int  lbm_frames_pending(const lbm_ctx* c);
/* Copies up to max_frames whole frames, oldest first, as [n][4][local_ny / k][nx / k] floats, their iterations into timesteps (may be
 * NULL), removes them from the ring and returns n. Synchronises. 0 when frames were never begun or none is pending. */
int  lbm_drain_frames(lbm_ctx* c, int* timesteps, float* frames, int max_frames);

/* ---- point probes with bilinear sampling (no reference counterpart: the reference writes whole fields, LBMIO.h:62-111; what this replaces
 * is a caller's lbm_get_macros — a synchronisation and 3 nx local_ny doubles over the bus — or a k = 1 frame — 4 nx local_ny floats —
 * per sample, to read a few dozen values) ----
 * A PROBE is a point (px, py) in GLOBAL lattice coordinates, given as doubles, 0 <= px <= nx - 1 and 0 <= py <= ny - 1. The SAMPLE of
 * iteration t at a probe is (rho, ux, uy) in double, interpolated bilinearly from the fine snapshot: cell for cell what lbm_get_macros
 * returns on a context with steps_done == t + 1 (the definition the statistics and the frames use; fp32 contexts widen to double first):
 *     x0 = floor(px), fx = px - x0, x1 = min(x0 + 1, nx - 1);   y likewise with ny - 1
 *     a = (1 - fx) v(x0, y0) + fx v(x1, y0);   b = (1 - fx) v(x0, y1) + fx v(x1, y1);   v = (1 - fy) a + fy b
 * Every product and every sum is rounded to double (no contraction). A cell whose weight is exactly zero is NOT read and its term is left
 * out: with fx == 0, a = v(x0, y0); with fy == 0, v = a. A probe on a lattice node therefore returns that cell's macros bit for bit and
 * reads no neighbour, in particular no ghost row. Solid cells enter with the (1, 0, 0) the snapshot gives them: documented, not corrected.
 * Strips: a probe belongs to the strip whose rows contain floor(py). The owner may read the ghost row next to its north face (y1) and,
 * for a probe in column 0 or nx - 1, the row beyond it, which the inlet / outlet cell pulls from: the rows the frame sample reads at the
 * same point of the schedule. Every other strip writes +0.0 for that probe: strips ADD UP like partial force sums. Every plan, layout,
 * arithmetic mode and decomposition gives the same bits for the same macros.
 * With probes active lbm_step / lbm_group_step append one sample to a device ring at exactly the iterations at which they append a
 * force-log row (output_frequency > 0 and t % output_frequency == 0), directly behind the force kernel (and the body, statistics and frame
 * samples), on the compute stream without a synchronisation; with the ring full they fail like the frame ring (LBM_ERR_ARG, "probe ring
 * full (%d samples): drain it (lbm_drain_probes)"). Probes change reporting only: populations, force logs, statistics, frames,
 * lbm_kernel_name and checkpoints (which do not carry probes) are those of a run without.
 * lbm_probes_begin: on an initialised context; xy = [n][2] GLOBAL coordinates (every strip of a run is given the same array),
 * 1 <= n <= LBM_PROBES_MAX, capacity >= 1 samples. Uploads a table {cell x0, local y0, fx, fy, owned} per probe and allocates the ring
 * (capacity x n x 3 doubles; the iterations stay on the host; freed by lbm_destroy). Calling it again replaces the table and empties the
 * ring; lbm_initialise empties the ring. LBM_ERR_ARG (the text names the offender): a null pointer, an uninitialised context, n < 1,
 * n > LBM_PROBES_MAX, capacity < 1, a coordinate that is not finite or lies outside the domain; LBM_ERR_ALLOC: no device memory for the ring. */
#define LBM_PROBES_MAX 65536
int  lbm_probes_begin(lbm_ctx* c, const double* xy, int n, int capacity);
/* Stops sampling and keeps the undrained samples. */
int  lbm_probes_end(lbm_ctx* c);
/* n of lbm_probes_begin; 0 without probes. */
int  lbm_probes_count(const lbm_ctx* c);
/* Samples in the ring that have not been drained (in a group: the same on every member). */
int  lbm_probes_pending(const lbm_ctx* c);
/* Copies up to max_samples whole samples, oldest first, as [m][n][3] doubles (rho, ux, uy; this strip's contribution: +0.0 for a probe
 * another strip owns), their iterations into timesteps (may be NULL), removes them from the ring and returns m. Synchronises. 0 when
 * probes were never begun or none is pending. */
int  lbm_drain_probes(lbm_ctx* c, int* timesteps, double* vals, int max_samples);

/* Debug/parity accessor: ghost-inclusive AoS [(local_ny+2)][(nx+2)][9] exactly as Grid::f_current /
 * Grid::f_next index it (LBMGrid.h:105-107,116-119). which: 0 = f_current, 1 = f_next. */
int  lbm_get_populations(lbm_ctx* c, int which, double* aos);
/* The write side of Grid::f_current (LBMGrid.h:115: `double& f_current(x,y,i)`): replaces the pre-collision state of the
 * next iteration by the interior cells of `aos` (same ghost-inclusive layout as lbm_get_populations; ghost entries are
 * ignored, they belong to the halo logic) and redoes collision_step() on it. Custom initial conditions enter here.
 * Until the next lbm_step the snapshots still show the values before the call. Synchronises. */
int  lbm_set_f_current(lbm_ctx* c, const double* aos);
/* Grid::is_solid (LBMGrid.h:146-148) for this strip, [local_ny][nx] bytes (the mask of lbm_set_solid_mask where one is set). */
int  lbm_get_solid(lbm_ctx* c, unsigned char* mask);
/* The write side of the geometry: generalises Grid::setup_geometry (LBMGrid.h:152-173), which marks the one disc of the
 * cylinder_* parameters, to any set of solid cells. `mask` is the GLOBAL [ny][nx] byte array, row y = 0 first (the layout of
 * lbm_get_solid); nonzero = solid. Every strip of a run is given the same global array and keeps the rows it can ever query (its
 * own +- 12 ghost rows). Call after lbm_create and before lbm_initialise, like the options (the plan is measured on this geometry);
 * from then on the cylinder_* parameters no longer define the geometry. The reference's semantics carry over unchanged: solid cells
 * hold w_i for ever, the collision and the wall / inlet / outlet conditions skip them, fluid cells pull w_i from solid neighbours,
 * forces are the momentum exchange over solid->fluid links (LBMSolver.h:84-265, LBMIO.h:133-168). lbm_get_solid, the solid count
 * of lbm_initialise, lbm_get_macros and the force log follow the mask; checkpoints carry its digest (lbm_save_state).
 * LBM_ERR_ARG: null pointer, nx / ny other than the domain's, or an initialised context. */
int  lbm_set_solid_mask(lbm_ctx* c, const unsigned char* mask, int nx, int ny);
/* The inflow: generalises the Zou-He velocity inlet (LBMSolver.h:181-206), which imposes inlet_velocity on every row, to one
 * x-velocity per row. `u` is the GLOBAL array of ny absolute lattice velocities, row y = 0 (bottom) first; no scaling is applied.
 * Every strip of a run is given the same global array. Call after lbm_create and before lbm_initialise, like lbm_set_solid_mask.
 * The reference's semantics carry over with u_in replaced by u[y] on row y: the wall rows still take bottom / top bounce-back first,
 * then the inlet; solid inlet cells are skipped; interior fluid cells of row y start at f_eq(1, (u[y], 0)) (evaluated on the host in
 * double, in the reference's bracket order), solid cells and the ghost frame as before; lbm_get_macros reports (rho_bc, u[y], 0) on
 * the inlet column and ux = u[y] in the initial snapshot. inlet_velocity then only names the run (checkpoint header, the
 * caller's Reynolds number). Checkpoints carry the profile's digest (lbm_save_state: magic "LBMCKPT3", flag bit 1).
 * LBM_ERR_ARG: null pointer, ny other than the domain's, an initialised context, or a value that is not finite or is >= 1 (the
 * inlet divides by 1 - u). */
int  lbm_set_inlet_profile(lbm_ctx* c, const double* u, int ny);
/* The inflow in time: generalises the Zou-He velocity inlet (LBMSolver.h:181-206), whose velocity is frozen for the whole run, to one
 * scale factor per iteration. No reference counterpart. A schedule is a table s[0..n) of doubles and a mode; iteration t — the absolute
 * loop-body number, the t of lbm_steps_done, continuing across checkpoints — takes
 *     LBM_INLET_HOLD   0   s(t) = s[min(t, n - 1)]   (ramps: the last entry holds for ever)
 *     LBM_INLET_REPEAT 1   s(t) = s[t mod n]         (periodic forcing)
 * and the inlet of iteration t imposes u_in = u[y] * s(t) on row y, u[y] being inlet_velocity or the profile of
 * lbm_set_inlet_profile. The table is cast once to the element type (memory: n elements on the device), and the product is ONE IEEE
 * multiplication in the element type, rounded before 1 - u_in and rho_bc * u_in use it, so strict and contracted arithmetic (option
 * "arith") apply the same bits in the inlet rule. Nothing else changes: the order bottom -> top -> inlet -> outlet on a cell stays, solid
 * inlet cells are skipped. Every fused level of a launch takes the factor of its own iteration, read on the device (a replayed graph
 * included). Negative factors are allowed: the inlet then acts as an outflow. The moving walls' velocity is not scaled, and a schedule
 * never differs per row.
 * Initial state: that of a context whose profile is u0[y] = u[y] * s[0], formed on the host in double — a ramp that starts at 0 starts
 * from rest, and the initial snapshot reports ux = u0[y]; the ghost frame is what it is with a profile. Snapshots (lbm_get_macros,
 * statistics, frames, probes, the f_current of lbm_get_populations) apply the inlet of the iteration they describe: a context with
 * lbm_steps_done == k >= 1 reports (rho_bc, u[y] * s(k - 1), 0) on the inlet column, the sample of output iteration t uses s(t).
 * Call after lbm_create and before lbm_initialise, in either order with lbm_set_inlet_profile: the plan is measured with the schedule
 * set. n == 0 clears the schedule. Every strip of a run is given the same schedule. The schedule changes no launch, no row range and no
 * exchange, and without one every result, kernel name, checkpoint byte and dry-run record is what it was without this call.
 * Checkpoints of a context with a schedule carry its digest (lbm_save_state: magic "LBMCKPT3", flag bit 5) and load only into
 * a context with an equal schedule; the iteration counter of the file positions the schedule after a restart.
 * LBM_ERR_ARG (the text names the offender, entry index included): a null context, an initialised context, n < 0 or
 * n > LBM_INLET_SCHEDULE_MAX, a null `s` with n > 0, a mode outside 0..1, an entry that is not finite. lbm_initialise, which knows
 * profile and schedule, fails with LBM_ERR_ARG naming row and entry unless u[y] * s[k] < 1 for every row and entry (the inlet divides by
 * 1 - u_in). */
#define LBM_INLET_HOLD 0
#define LBM_INLET_REPEAT 1
#define LBM_INLET_SCHEDULE_MAX 1048576
int  lbm_set_inlet_schedule(lbm_ctx* c, const double* s, int n, int mode);
/* The length of the schedule as set; 0 without one (or for a null context). */
int  lbm_inlet_schedule_length(const lbm_ctx* c);
/* The factor iteration t applies, as the kernels see it: (double)(T)s(t) in the element type T; 1.0 without a schedule.
 * LBM_ERR_ARG: null argument, t < 0. */
int  lbm_get_inlet_scale(const lbm_ctx* c, int t, double* s_out);
/* The collision: replaces the BGK operator's one global tau (LBMSolver.h:85) by a Smagorinsky subgrid model with constant `cs`. Each
 * fluid cell relaxes with tau_eff = (tau + sqrt(tau^2 + 18 sqrt(2) cs^2 |Pi|/rho)) / 2, where Pi is the non-equilibrium momentum flux
 * of its post-BC populations: the closed form of tau_eff = tau + 3 cs^2 |S|, |S| = sqrt(2 S:S), for cs^2 = 1/3 and dx = dt = 1. This
 * stabilises runs whose tau approaches 0.5 (higher Reynolds numbers on the same grid); tau (and with it the caller's Reynolds number)
 * keeps naming the molecular viscosity. Strict arithmetic (option arith=0) evaluates the operator in IEEE operations with correctly
 * rounded square roots, contracted arithmetic (arith=1) with FMAs. Every strip of a run is given the same value. Call after lbm_create
 * and before lbm_initialise, like lbm_set_solid_mask: the plan is then measured on the LES kernels (no fp32 deep=8 plan: pinning it
 * fails). cs == 0 clears the model (the BGK kernels). Checkpoints carry cs (lbm_save_state: magic "LBMCKPT3", flag bit 2).
 * LBM_ERR_ARG: null context, an initialised context, a value that is not finite, < 0 or > 1, or a nonzero value on a context with a
 * TRT magic parameter (lbm_set_trt): the two collisions cannot be combined. */
int  lbm_set_smagorinsky(lbm_ctx* c, double cs);
/* The collision: replaces the single-relaxation-time BGK operator by the two-relaxation-time one (TRT: Ginzburg, d'Humieres) with
 * "magic" parameter `magic` = (tau - 1/2)(tau_minus - 1/2). With feq as BGK forms it, the rest population relaxes with wp = 1/tau, and
 * each opposite pair (i, ib) of (1,3), (2,4), (5,7), (8,6) is split into its even and odd non-equilibrium parts,
 *     np = ((f_i + f_ib) - (feq_i + feq_ib)) / 2,  nm = ((f_i - f_ib) - (feq_i - feq_ib)) / 2,
 *     f_i' = f_i - wp np - wm nm,  f_ib' = f_ib - wp np + wm nm,     wp = 1 / tau,  wm = 1 / (1/2 + magic / (tau - 1/2)).
 * The even rate sets the viscosity, (tau - 1/2) / 3 as before; the odd rate is free, and with magic fixed the place of a bounce-back
 * wall no longer moves with the viscosity. magic = 1/4 is the most stable choice, 3/16 puts the wall of a straight channel exactly
 * half-way; magic = (tau - 1/2)^2 makes the two rates equal (BGK up to rounding). Both rates are computed in double and cast to the
 * element type. Strict arithmetic (option arith=0) evaluates the lines above operation by operation in IEEE arithmetic, contracted
 * arithmetic (arith=1) with FMAs. No extra memory traffic. Every strip of a run is given the same value. Call after lbm_create and
 * before lbm_initialise, like lbm_set_smagorinsky: the plan is then measured on the TRT kernels (no fp32 deep=8 plan: pinning it fails).
 * magic == 0 clears the model (the BGK kernels). Checkpoints carry magic (lbm_save_state: magic word "LBMCKPT3", flag bit 3).
 * LBM_ERR_ARG: null context, an initialised context, a value that is not finite, < 0 or > 1, a context whose tau <= 0.5, or a
 * context with a nonzero Smagorinsky constant: the two collisions cannot be combined. */
int  lbm_set_trt(lbm_ctx* c, double magic);
/* The collision: a uniform driving force. A constant force density F = (fx, fy) in lattice units acts on every fluid cell at every
 * iteration: the pressure-gradient-equivalent drive of a channel, gravity, a cross-stream force on a wake. ("Forcing", because "body
 * forces" are the momentum-exchange forces on obstacles: lbm_get_body_forces.) The scheme is Guo, Zheng and Shi (2002) on the BGK
 * operator: the equilibrium is taken at the velocity u = (sum_i c_i f_i + F/2) / rho, and the source
 *     S_i = (1 - 1/(2 tau)) w_i [3 (c_i - u) + 9 (c_i . u) c_i] . F
 * is added to the relaxed populations, f_i' = (f_i - (f_i - feq_i(rho, u)) / tau) + S_i. The host forms the launch-uniform values in
 * double and casts each once to the element type: wp = 1/tau, g = (1 - wp/2) F, h = F/2. Strict arithmetic (option arith=0) evaluates,
 * one IEEE operation at a time with no contraction: the sums rho, jx, jy of BGK; jx + hx, jy + hy; the two divisions by rho; feq_i as
 * BGK forms it from these ux, uy; u3 = 3 (ux gx + uy gy); S_0 = w_0 (0 - u3); and per opposite pair (i, ib) of (1,3), (2,4), (5,7),
 * (8,6), with cu as BGK's and cg = gx, gy, gx + gy, gx - gy: a = 3 cg, b = (9 cu) cg, S_i = w_i ((a - u3) + b),
 * S_ib = w_i ((-a - u3) + b). Contracted arithmetic (arith=1) folds the source into its FMA chain. The sum of the S_i is zero (mass is
 * kept) and a collision adds exactly F to a cell's momentum. No extra memory traffic.
 * Every cell that collides today takes the force: the cells of the wall rows and of the inlet and outlet columns included.
 * The snapshot — lbm_get_macros, statistics, frames, probes — reports Guo's velocity on the interior fluid cells of a forced context,
 * through the one function they share: the populations it reads are post-collision ones, whose momentum is the pre-collision one plus
 * F, so it forms (sum_i c_i f_i - F/2) / rho, one IEEE subtraction per component before the division. The inlet and outlet columns,
 * solid cells and the initial snapshot report what they report without a force.
 * Unchanged: the momentum-exchange forces on obstacles, the stability scan, the halo exchange, every launch and row range and the
 * dry-run choreography (lbm_debug_choreography); with (0, 0) every result, kernel name and checkpoint byte is what it was without this
 * call. Documented, not corrected: the Zou-He inlet and outlet, the wall rules and the solid cells do not know about the force (the
 * boundary rules prescribe their velocity and density as they do without one, and bounce-back is not force-corrected).
 * Call after lbm_create and before lbm_initialise, like lbm_set_trt: the plan is then measured on the forced kernels (Arith values
 * 8 / 9; no fp32 deep=8 plan: pinning it fails). Every strip of a run is given the same values. (0, 0) clears the model (the BGK
 * kernels). Checkpoints carry the force (lbm_save_state: magic "LBMCKPT3", flag bit 6) and load only into a context with an
 * equal one.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, a component that is not finite or has
 * magnitude >= 1, or a nonzero force on a context with a Smagorinsky constant or a TRT magic parameter — and either of those on a
 * context with a force: the collisions cannot be combined. */
int  lbm_set_forcing(lbm_ctx* c, double fx, double fy);
/* The force as set, (0, 0) on a context without one; either pointer may be NULL. LBM_ERR_ARG: null context. */
int  lbm_get_forcing(const lbm_ctx* c, double* fx, double* fy);
/* The collision: replaces the BGK operator by a multiple-relaxation-time one (MRT: Lallemand and Luo 2000, d'Humieres 2002) whose bulk
 * rate `bulk_rate` = sb is free of tau, in the pair form of lbm_set_trt plus that one rate. With feq as BGK forms it, n0 = f0 - feq0 and,
 * per opposite pair p = (i, ib) of (1,3), (2,4), (5,7), (8,6), TRT's even and odd non-equilibrium parts np_p, nm_p:
 *     ta = (np_13 + np_24) / 2,  da = (np_13 - np_24) / 2       (axis pairs: trace and deviator)
 *     td = (np_57 + np_86) / 2,  dd = (np_57 - np_86) / 2       (diagonal pairs)
 *     f0' = f0 - sb n0
 *     f1' = f1 - (sb ta + wp da) - wm nm_13,  f3' = f3 - (sb ta + wp da) + wm nm_13
 *     f2' = f2 - (sb ta - wp da) - wm nm_24,  f4' = f4 - (sb ta - wp da) + wm nm_24
 *     f5' = f5 - (sb td + wp dd) - wm nm_57,  f7' = f7 - (sb td + wp dd) + wm nm_57
 *     f8' = f8 - (sb td - wp dd) - wm nm_86,  f6' = f6 - (sb td - wp dd) + wm nm_86
 *     wp = 1 / tau,  wm = 1 / (1/2 + magic / (tau - 1/2)).
 * In moment space (rho, e, eps, jx, qx, jy, qy, pxx, pxy) this is the Lallemand-Luo operator with the rates (0, sb, sb, 0, wm, 0, wm, wp,
 * wp): the shear viscosity stays (tau - 1/2) / 3, the bulk viscosity grows with 1/sb - 1/2, and mass and momentum are conserved, so the
 * snapshot (lbm_get_macros, statistics, frames, probes) needs no correction. sb = 1/tau is TRT with the same magic up to rounding, and
 * magic = (tau - 1/2)^2 besides is BGK up to rounding. The host forms sb, wp, wm in double and casts each once to the element type.
 * Strict arithmetic (option arith=0) evaluates, one IEEE operation at a time with no contraction: rho, ux, uy and the feq_i as BGK forms
 * them; f0' = f0 - sb (f0 - feq0); per pair np = 0.5 ((f_i + f_ib) - (feq_i + feq_ib)), nm = 0.5 ((f_i - f_ib) - (feq_i - feq_ib)),
 * o = wm nm; per group (p, q) of pairs, (13, 24) and (57, 86): t = 0.5 (np_p + np_q), d = 0.5 (np_p - np_q), a = sb t, b = wp d,
 * e_p = a + b, e_q = a - b; then f_i' = (f_i - e_p) - o_p, f_ib' = (f_ib - e_p) + o_p for pair p and the same with e_q, o_q for pair q.
 * Contracted arithmetic (arith=1) is TRT's FMA chain on an equilibrium whose velocity-free term is shifted, for the axis pairs and for the diagonal pairs, so that each population takes (sb - wp)/4 times the sum of its group's residuals. About a
 * dozen operations per cell more than TRT, no extra memory traffic. Every strip of a run is given the same pair.
 * Call after lbm_create and before lbm_initialise, like lbm_set_trt: the plan is then measured on the MRT kernels (Arith values 16 / 17;
 * no fp32 deep=8 plan: pinning it fails). bulk_rate == 0 clears the model: the BGK kernels, and every result, kernel name and checkpoint
 * byte as without the call (magic is then ignored, if finite). Checkpoints carry the pair (lbm_save_state: magic word "LBMCKPT3", flag
 * bit 10) and load only into a context with an equal one.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, a value that is not finite, a nonzero bulk_rate
 * outside (0, 2), magic outside (0, 1] with a nonzero bulk_rate, a context whose tau <= 0.5, or a context with a Smagorinsky constant,
 * a TRT magic parameter or a force — and any of those setters on a context with MRT: the collisions cannot be combined. */
int  lbm_set_mrt(lbm_ctx* c, double bulk_rate, double magic);
/* The pair as set, (0, 0) on a context without MRT; either pointer may be NULL. LBM_ERR_ARG: null context. */
int  lbm_get_mrt(const lbm_ctx* c, double* bulk_rate, double* magic);
/* The collision: an outlet sponge zone (a viscosity sponge) in front of the east port. Over the last `width` columns the relaxation time
 * rises smoothly from tau to `tau_end`, so that vortices and pressure waves are diffused before they meet the port, which reflects them.
 * With x0 = nx - 1 - width:
 *     column x <= x0:  tau_x = tau                                       (its rate is the very bits BGK's 1/tau holds)
 *     column x >  x0:  tau_x = tau + (tau_end - tau) * (s * s),  s = (double)(x - x0) / (double)width
 * formed on the host in double, in exactly that order; the kernels read the table wp_x[x] = (T)(1.0 / tau_x), cast once to the element
 * type, nx elements. The collision is BGK's with 1/tau replaced by wp_x of the cell's column: strict arithmetic (option arith=0)
 * evaluates f_i - wp_x (f_i - feq_i) operation by operation as BGK does, contracted arithmetic (arith=1) BGK's FMA chain with that rate.
 * Every cell that collides takes its column's rate, the port columns and the wall rows included; solid cells are skipped as ever. BGK
 * conserves mass and momentum at any rate, so the snapshot (lbm_get_macros, statistics, frames, probes) needs no correction. The ports
 * and the walls do not know about the sponge, and the viscosity inside the zone is (tau_x - 1/2) / 3: results taken there are not those
 * of the fluid. The register kernel reads its column's rate once per launch; no extra memory traffic per cell.
 * Call after lbm_create and before lbm_initialise, like lbm_set_mrt: the plan is then measured on the sponge kernels (Arith values
 * 32 / 33; neither the fp32 64x48 nor the fp64 64x40 regions: pinning them fails). width == 0 clears the model: the BGK kernels, and every
 * result, kernel name, plan candidate and checkpoint byte as without the call (tau_end is then ignored). Every strip of a run is given
 * the same pair; strips cut rows, so every strip holds the whole table. Forces, the stability scan, the halo exchange and every launch
 * and row range are those of BGK. Checkpoints carry the pair (lbm_save_state: magic word "LBMCKPT3", flag bit 11) and load only into a
 * context with an equal one.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, width < 0 or width > nx - 1 (column 0 keeps tau),
 * with a nonzero width a tau_end that is not finite or is <= 0.5 or a context whose tau <= 0.5, or a context with a Smagorinsky
 * constant, a TRT magic parameter, a force or MRT — and any of those setters on a context with a sponge: the collisions cannot be
 * combined. */
int  lbm_set_sponge(lbm_ctx* c, int width, double tau_end);
/* The pair as set, (0, 0) on a context without a sponge; either pointer may be NULL. LBM_ERR_ARG: null context. */
int  lbm_get_sponge(const lbm_ctx* c, int* width, double* tau_end);
/* The rate column x relaxes with, as the kernels see it: (double)(T)(1 / tau_x); BGK's (double)(T)(1 / tau) without a sponge.
 * LBM_ERR_ARG: a null context or pointer, x outside 0 .. nx - 1. */
int  lbm_get_sponge_rate(const lbm_ctx* c, int x, double* wp_out);
/* The two walls: generalises the on-node bounce-back of the bottom and top rows (LBMSolver.h:155-176), a stationary no-slip wall, to a
 * KIND and a tangential VELOCITY per wall. The south wall is global row 0, the north wall global row ny - 1. On a fluid cell of the
 * wall's row, after the pull:
 *     kind                   south wall                          north wall
 *     LBM_WALL_NOSLIP   0    f2 = f4; f5 = f7;     f6 = f8       f4 = f2; f7 = f5;     f8 = f6        (the reference's; the default)
 *     LBM_WALL_FREESLIP 1    f2 = f4; f5 = f8;     f6 = f7       f4 = f2; f7 = f6;     f8 = f5        (specular reflection)
 *     LBM_WALL_MOVING   2    f2 = f4; f5 = f7 + k; f6 = f8 - k   f4 = f2; f7 = f5 - k; f8 = f6 + k    (k = velocity / 6)
 * k is the momentum correction 6 w_i rho_w (c_i . u_w) of a diagonal population with rho_w = 1, formed once on the host in double and
 * cast to the element type; each corrected population is ONE IEEE addition, so strict and contracted arithmetic (option "arith") apply
 * the same bits in the wall rule. Every kind leaves the pair sums, and with them mass, as bounce-back does. Everything else stays the
 * reference's: the sequential order bottom -> top -> inlet -> outlet on a cell (a corner cell takes the wall rule first, then Zou-He,
 * which reads the populations the wall has just written); solid cells of a wall row are skipped; the ghost rows keep their permanent
 * content; the initial state is unchanged (interior cells start at the inlet equilibrium). The snapshot — lbm_get_macros, statistics,
 * frames, probes — applies the same rule through the same function, and so does the f_current of lbm_get_populations.
 * Documented, not corrected: the on-node scheme does not make ux on a moving wall's row equal to the wall's velocity (the row's
 * populations are collided like any other's), and rho_w is 1, not the local density. A free-slip wall grows no boundary layer: a
 * uniform stream stays uniform (unconfined flow past a body); a moving wall drives Couette flow, a lid, a ground plane.
 * Call after lbm_create and before lbm_initialise, like lbm_set_inlet_profile: the plan is measured with the walls set. Every strip of
 * a run is given the same two walls; a strip that holds neither row 0 nor row ny - 1 carries the values and never uses them. The walls
 * change no launch and no row range: forces, body forces, the halo exchange and the dry-run choreography (lbm_debug_choreography) are
 * untouched, and with kind 0 on both walls every result, kernel name and checkpoint byte is what it was without this call.
 * `velocity` is read for LBM_WALL_MOVING only and must be 0 for the other kinds; setting LBM_WALL_NOSLIP clears a wall. Checkpoints
 * carry both walls where either is not no-slip (lbm_save_state: magic "LBMCKPT3", flag bit 4) and load only into a context with equal
 * walls.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, side outside 0..1, kind outside 0..2, a
 * velocity that is not finite or has |velocity| >= 1, a nonzero velocity with kind 0 or 1. */
#define LBM_WALL_SOUTH 0
#define LBM_WALL_NORTH 1
#define LBM_WALL_NOSLIP   0
#define LBM_WALL_FREESLIP 1
#define LBM_WALL_MOVING   2
int  lbm_set_wall(lbm_ctx* c, int side, int kind, double velocity);
/* The wall of `side` as set (kind 0, velocity 0 on a fresh context); either pointer may be NULL. LBM_ERR_ARG: null context, side outside 0..1. */
int  lbm_get_wall(const lbm_ctx* c, int side, int* kind, double* velocity);
/* The two ports: generalises the two open ends of the channel (LBMSolver.h:181-235), a Zou-He velocity inlet on column 0 and a Zou-He
 * pressure outlet with rho = 1 on column nx - 1, to a KIND and a VALUE per end. The west port is column 0, the east port column
 * nx - 1. On a fluid cell of the port's column, after the pull and after the wall rule, in the unchanged order bottom -> top -> west ->
 * east:
 *     west   S = f0 + f2 + f4 + 2 (f3 + f6 + f7)
 *       LBM_PORT_VELOCITY 0   u = u[y] * s(t) (inlet_velocity / lbm_set_inlet_profile / lbm_set_inlet_schedule), rho = S / (1 - u)  (the default)
 *       LBM_PORT_PRESSURE 1   rho = value, u = 1 - S / rho
 *       then f1 = f3 + (2/3) rho u;  f5 = f7 - 0.5 (f2 - f4) + (1/6) rho u;  f8 = f6 + 0.5 (f2 - f4) + (1/6) rho u
 *     east   S = f0 + f2 + f4 + 2 (f1 + f5 + f8)
 *       LBM_PORT_PRESSURE 1   rho = value, u = -1 + S / rho                                                     (the default, with value 1)
 *       LBM_PORT_VELOCITY 0   u = value,   rho = S / (1 + u)
 *       then f3 = f1 - (2/3) rho u;  f6 = f8 - 0.5 (f2 - f4) - (1/6) rho u;  f7 = f5 + 0.5 (f2 - f4) - (1/6) rho u
 * The value is cast once to the element type; every operation is one IEEE operation in that type in the order written, (2/3) * rho * u
 * from left to right, so strict and contracted arithmetic (option "arith") apply the same bits in the port rule. With the defaults, west
 * (VELOCITY, 0) and east (PRESSURE, 1.0), S / 1 and 1 * u change no bit: every result, kernel name, checkpoint byte and dry-run record
 * is what it was without this call. Flow driven by a density difference is (PRESSURE, rho_w) and (PRESSURE, rho_e) with
 * inlet_velocity = 0; suction or a piston is an east VELOCITY port (u > 0 leaves the domain).
 * Everything else stays the reference's: solid cells of a port column are skipped; with nx == 1 the west rule runs first, then the east
 * rule on the same cell; the initial state is unchanged (interior cells start at f_eq(1, (u[y] s(0), 0)) of inlet_velocity, profile and
 * schedule), and so are the ghost frame, the reference velocity of Cd / Cl (inlet_velocity), the forces, the stability scan, the halo
 * exchange and the dry-run choreography: the ports change no launch and no row range. The snapshot - lbm_get_macros, statistics, frames,
 * probes - reports (rho, u, 0) of the rule on a port column, through the same function: the given one as cast, the other as solved; so
 * does the f_current of lbm_get_populations. A schedule scales the west velocity only, never a pressure or the east velocity.
 * Documented, not corrected: the rules do not know about a driving force (lbm_set_forcing), like the reference's pair; and they are not
 * mass-tight at the reference's walls: the on-node walls exchange mass with the fluid wherever rho is not 1, so the flux of a
 * pressure-driven channel is not constant along x.
 * Call after lbm_create and before lbm_initialise, like lbm_set_wall: the plan is measured with the ports set. Every strip of a run is
 * given the same two ports. A west PRESSURE port takes no inlet velocity: lbm_initialise fails with LBM_ERR_ARG, naming the offender, if
 * an inlet profile or an inlet schedule is set beside it. Checkpoints carry both ports where either is off its default (lbm_save_state:
 * magic "LBMCKPT3", flag bit 8) and load only into a context with equal ports.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, side outside 0..1, kind outside 0..1, a value
 * that is not finite, a pressure <= 0, an east velocity with |u| >= 1, a nonzero value with west VELOCITY. */
#define LBM_PORT_WEST 0      /* column 0 */
#define LBM_PORT_EAST 1      /* column nx - 1 */
#define LBM_PORT_VELOCITY 0
#define LBM_PORT_PRESSURE 1
int  lbm_set_port(lbm_ctx* c, int side, int kind, double value);
/* The port of `side` as set (west: kind 0, value 0; east: kind 1, value 1 on a fresh context); either pointer may be NULL. LBM_ERR_ARG: null context, side outside 0..1. */
int  lbm_get_port(const lbm_ctx* c, int side, int* kind, double* value);

/* ---- periodic top and bottom boundaries (periodic y) ----
 * on = 1: the lattice is the ny rows repeated for ever. Row -1 is row ny - 1 and row ny is row 0, for the populations, for the geometry
 * - solid(x, y) = S(x, y mod ny) with S what lbm_get_solid returns, disc or mask - and for the inlet profile, u[y mod ny]. No wall rule
 * runs anywhere: a fluid cell of row 0 or ny - 1 takes its nine pulls, then the port rules if it lies on column 0 or nx - 1 (west, then
 * east, as ever). Everything else is the reference's: solid cells, the stability scan, the initial state, zeros in the E/W ghost columns
 * (those of the wrapped rows included). Forces cross the seam: a fluid cell (x, y) whose neighbour (x + cx, (y + cy) mod ny) is solid
 * contributes 2 c_i f_i, to the strip that owns the fluid cell. Snapshots (macros, statistics, probes) are per cell what they were;
 * frames take the central difference for d/dy on rows 0 and ny - 1, with the wrapped neighbour (the x edges keep the one-sided form).
 * Probe coordinates stay 0 <= py <= ny - 1: there is no interpolation across the seam.
 * A periodic context is a strip with two live faces: it uses the row-interleaved layout and the strip plans, and wraps through device
 * copies of its own edge rows into its own ghost rows after every launch (the halo exchange of a strip, with itself as both
 * neighbours). In a group (lbm_group_link) strip 0 and strip n - 1 become neighbours on either transport. It is never a whole domain
 * for the plans: pinning "split", a whole-domain-only shape ("deep" 10, 11: the fp64 64x40 regions) or "layout" 0 makes lbm_initialise fail with
 * LBM_ERR_ARG, naming the option. ny >= 2 * LBM_HALO_ROWS, like any strip with neighbours.
 * lbm_initialise also refuses, naming the offender: a wall that is not no-slip (lbm_set_wall) beside periodic y; body labels
 * (lbm_set_body_labels) with a labelled cell on row 0 or ny - 1 (the per-body boxes are clipped at the domain, so such a body's links
 * across the seam would be missed; bodies away from the seam work); a communicator of more than one rank (lbm_comm_init: rings of
 * processes are not built). lbm_halo_export / lbm_halo_import refuse a periodic context. Checkpoints carry the setting (lbm_save_state:
 * magic "LBMCKPT3", flag bit 9, no payload) and load only into a context with the same setting.
 * Without the call, or with on = 0, every result, kernel name, plan candidate, checkpoint byte and dry-run record is what it was.
 * lbm_set_option(c, "periodic_y", on) is the same call. Call after lbm_create and before lbm_initialise.
 * LBM_ERR_ARG (the text names the offender): a null context, an initialised context, on outside 0..1. */
int  lbm_set_periodic_y(lbm_ctx* c, int on);
/* 1 on a periodic context, else 0; 0 for a null context. */
int  lbm_get_periodic_y(const lbm_ctx* c);

/* ---- strip halo exchange (replaces Grid::exchange_ghost_cells, LBMGrid.h:249-283) ----
 * Device path: RCCL send/recv of the LBM_HALO_ROWS edge rows per face (one contiguous run in the row-interleaved
 * layout) once per launch of up to six iterations (or 2 x LBM_HALO_ROWS rows once per two such launches: option "deep_halo" 2,
 * measured at lbm_initialise), on a side stream, overlapped with the interior update. `id128` is the 128-byte
 * ncclUniqueId produced by lbm_comm_unique_id on rank 0 and distributed by the launcher. Ranks are ordered bottom (0)
 * to top; attach the communicator before lbm_initialise. */
int  lbm_comm_unique_id(void* id128);
int  lbm_comm_init(lbm_ctx* c, int rank, int nranks, const void* id128);
/* Sum the partial force sums / max / min across strips (the reference's MPI_Reduce/MPI_Allreduce at
 * LBMIO.h:167-168, LBMGrid.h:315,342). In place, host values, n doubles. op: 0 sum, 1 max, 2 min. */
int  lbm_comm_allreduce(lbm_ctx* c, double* vals, int n, int op);
/* In-process strips (replaces the decomposition Grid::initialise_2d_topology builds, LBMGrid.h:347-392, when ONE process
 * drives several GPUs, e.g. `lbm_solver --gpus 8`): n contexts created for consecutive strips (bottom to top, covering
 * all ny rows; any devices) are linked into a group and then initialised and stepped together by the calling thread.
 * transport 0: every strip pulls its neighbours' edge rows with hipMemcpyPeerAsync over xGMI (plain device copies when
 * two strips share a device) on its side stream, behind the neighbour's edge-rows event; transport 1: RCCL, one
 * communicator per member (ncclCommInitAll; distinct devices), all members' ncclSend/ncclRecv in one group call.
 * The launch sequence, the exchange cadence and the overlap are those of lbm_step. The results of the whole lattice are read
 * through the gathers below (lbm_group_get_* / lbm_group_drain_*); the per-member entry points keep returning a strip's part.
 * lbm_group_refresh_halos: after lbm_load_state on every member.
 * Errors: a member's failure (or LBM_ERR_TIMEOUT: a strip thread that did not reach a rendezvous within "wait_timeout_ms") makes
 * lbm_group_step return that error on the caller with every strip thread parked again; the launch in flight was abandoned half-way,
 * so the populations are undefined until lbm_group_initialise (or lbm_load_state + lbm_group_refresh_halos) — after a time-out the
 * group refuses further work and is only good for lbm_destroy. */
int  lbm_group_link(lbm_ctx** ctxs, int n, int transport);
int  lbm_group_initialise(lbm_ctx** ctxs, int n, int* solid_total_out);
int  lbm_group_step(lbm_ctx** ctxs, int n, int nsteps, int output_frequency);
int  lbm_group_refresh_halos(lbm_ctx** ctxs, int n);
/* The gathers of a group: every result of the per-member entry points put together for the WHOLE lattice, in one place (replaces the
 * gathers of the reference's Solver / IOManager across its ranks: MPI_Gatherv of the fields, LBMSolver.h:340-357, MPI_Reduce(SUM) of the
 * forces, LBMIO.h:167-168, MPI_Allreduce(MIN / MAX) of the stability flag and max|u|, LBMGrid.h:315,342). ctxs / n: the group as linked
 * (LBM_ERR_ARG otherwise); one linked or unlinked whole-domain context (n == 1) is a group. Each call runs the member's entry point of
 * the same name on member 0, 1, .. n-1 in turn on the calling thread and returns its first error; arrays are those of the member call
 * with ny in place of local_ny. The rules (csrc/lbm_gather.hpp; lbm_debug_gather runs them without a device):
 *   ROWS   a plane of a member lies at row y_start of the plane of the whole lattice (a frame's at row y_start / k);
 *   SUM    strip 0's value, then += the values of strips 1 .. n-1 in that order, for forces, body forces and probes alike. There is no
 *          leading 0 +: a sum whose only terms are -0.0 is -0.0 (a caller that starts from 0.0 gets +0.0; nonzero sums are the same bits);
 *   COUNT  a count every member must hold alike is returned as that value; LBM_ERR_ARG "... disagree ..." if the members differ.
 * ALL OR NOTHING: a drain compares, before the first member is drained, what the host knows without a device call — every member's
 * number of pending samples and, for frames and probes, the iteration of each sample it would take — and on a difference returns
 * LBM_ERR_ARG "... disagree ..." with every ring as it was. (They are equal whenever lbm_group_step was the only thing that stepped the
 * members.) The two force logs keep their iterations in device memory: those are compared row by row after the copy, and a difference
 * there is reported as LBM_ERR_ARG "... disagree ... the drained rows are gone". */
int  lbm_group_first_unstable_step(lbm_ctx** ctxs, int n, int* t_out);    /* min over the members that report a step; -1 if none does */
int  lbm_group_max_velocity_sq(lbm_ctx** ctxs, int n, double* out);       /* max over the members */
int  lbm_group_get_forces(lbm_ctx** ctxs, int n, double* fx, double* fy); /* SUM */
/* Every row of the members' force logs, the partial sums added per row (SUM); the members' row counts and the iteration of every row
 * must agree. Like lbm_drain_force_log it returns every row, or LBM_ERR_ARG "force log holds %d rows, buffer takes %d" with nothing drained. */
int  lbm_group_drain_force_log(lbm_ctx** ctxs, int n, lbm_force_row* rows, int max_rows);
int  lbm_group_get_body_forces(lbm_ctx** ctxs, int n, double* fxy);       /* [B][2], SUM */
/* Whole samples of B rows, as many as fit into max_rows, summed per row like the force log; returns the ROWS copied, 0 without labels. */
int  lbm_group_drain_body_force_log(lbm_ctx** ctxs, int n, lbm_body_force_row* rows, int max_rows);
/* [ny][nx] each (any may be NULL); every member writes its rows into place (ROWS), without a staging copy. */
int  lbm_group_get_macros(lbm_ctx** ctxs, int n, double* rho, double* ux, double* uy);
/* [(ny+2)][(nx+2)][9]: every member gives its interior rows, member 0 also the south physical ghost row, member n-1 the north one. */
int  lbm_group_get_populations(lbm_ctx** ctxs, int n, int which, double* aos);
int  lbm_group_stats_samples(lbm_ctx** ctxs, int n);                      /* COUNT */
int  lbm_group_get_stat_sums(lbm_ctx** ctxs, int n, double* sums6);       /* [6][ny][nx], ROWS */
/* The inverse of lbm_group_get_stat_sums: every member is given its rows of sums6 = [6][ny][nx] and the sample count. */
int  lbm_group_stats_restore(lbm_ctx** ctxs, int n, const double* sums6, int samples);
int  lbm_group_frames_pending(lbm_ctx** ctxs, int n);                     /* COUNT (the pending iterations must agree too) */
int  lbm_group_probes_pending(lbm_ctx** ctxs, int n);                     /* COUNT (likewise) */
/* Up to max_frames whole frames, oldest first, as [m][4][ny / k][nx / k] floats (ROWS at y_start / k; k must be the same on every
 * member), their iterations into timesteps (may be NULL); returns m; 0 when frames were never begun or none is pending. */
int  lbm_group_drain_frames(lbm_ctx** ctxs, int n, int* timesteps, float* frames, int max_frames);
/* Up to max_samples whole samples, oldest first, as [m][probes][3] doubles (SUM; the number of probes must be the same on every member),
 * their iterations into timesteps (may be NULL); returns m; 0 when probes were never begun or none is pending. */
int  lbm_group_drain_probes(lbm_ctx** ctxs, int n, int* timesteps, double* vals, int max_samples);
/* What this process actually bound at run time (another library loaded first may have brought its own RCCL / HIP):
 * ncclGetVersion, hipRuntimeGetVersion, hipDriverGetVersion. Any pointer may be NULL. */
int  lbm_runtime_versions(int* rccl, int* hip_runtime, int* hip_driver);
/* hipMemGetInfo of a device (leak checks; sizing of strips). Any pointer may be NULL. */
int  lbm_device_memory(int device, unsigned long long* free_bytes, unsigned long long* total_bytes);
/* The exchange schedule of a strip with a communicator ("overlap=.. deep_halo=.. (..)"): measured at lbm_initialise
 * over the four schedules (collective; MAX over the ranks) unless pinned with lbm_set_option. */
const char* lbm_strip_schedule(const lbm_ctx* c);
/* Host-staged path (the buffers the reference hands to MPI_Isend/Irecv, LBMGrid.h:255-276). Each face buffer is
 * [LBM_HALO_ROWS][9][nx] doubles: the LBM_HALO_ROWS (= 6) interior rows next to that face, bottom row first, all nine
 * populations (six rows: one launch of up to six fused iterations — or two launches of up to three, the first one
 * recomputing three of the neighbour's rows — may run between two exchanges).
 * export: south_out = my bottom rows, north_out = my top rows; import: south_in -> my south ghost rows (= the south
 * neighbour's north_out), north_in -> my north ghost rows. NULL = that side is a physical wall. The caller exchanges
 * after lbm_initialise and after EVERY lbm_step call, and calls lbm_step so that it issues at most TWO launches
 * (e.g. nsteps <= 4 by default = a fused launch of three iterations + a single one, or nsteps = 6 with the option
 * "trailing_pair" 1; with a "deep" plan ONE launch of up to six iterations; lbm_step refuses a call that would need
 * more). Used by
 * MPI-hosted callers and by the 2-rank tests. */
#define LBM_HALO_ROWS 6
int  lbm_halo_export(lbm_ctx* c, double* south_out, double* north_out);
int  lbm_halo_import(lbm_ctx* c, const double* south_in, const double* north_in);

/* Checkpoint / restart (the reference has none): the strip's post-collision populations and the
 * iteration counter. lbm_load_state needs an initialised context created with the same parameters; the macro /
 * population snapshots become available again after the next lbm_step. A file written with an obstacle mask, an inlet
 * profile, a Smagorinsky constant, a TRT magic parameter, a force (lbm_set_forcing), an MRT pair (lbm_set_mrt), an outlet sponge (lbm_set_sponge), a wall that is not no-slip (lbm_set_wall), an
 * inlet schedule (lbm_set_inlet_schedule) or a port off its default (lbm_set_port) loads only into a context with the same mask,
 * profile, constant, parameter, force, walls, schedule and ports (the failure names which one differs). The file format, and the order in which differences are named: the comment at the
 * head of csrc/lbm_ckpt.hpp. */
int  lbm_save_state(lbm_ctx* c, const char* path);
int  lbm_load_state(lbm_ctx* c, const char* path);

/* Tuning/diagnostics (not part of the reference surface). Keys, all to be set before lbm_initialise:
 *   "tune" 1|0    time the candidate plans at lbm_initialise and keep the fastest (default 1); with 0 the plan is
 *                 "layout" 0 planar|1 row-interleaved,
 *                 "nt" non-temporal stores, "ntl" non-temporal level-1 loads of the register kernel ("deep" 6 / 7),
 *                 "alternate" alternate the row walk direction per launch,
 *                 "fuse" 1|2|3|4 iterations fused per launch through LDS (k_step2_tile / k_step3_tile / k_step4_tile, the
 *                 last only for a context without strip faces;
 *                 "pair" 1 == "fuse" 2), "pair_ty" 8|12 tile height, "xcd" XCD-aware tile walk,
 *                 "trailing_pair" 1 lets an lbm_step call end on a fused launch (snapshots then need one more step)
 *                 "deep" 1..3, 6..11: more iterations per launch. 1 / 2 / 3: six / seven / eight iterations on an LDS-filling
 *                 64x16 / 64x16 / 32x32 tile (k_stepd_tile, 1024-thread blocks: grids of a single round of blocks); 6 / 7:
 *                 five / six iterations with the lattice of a 64x32 region held in registers (k_stepc_col, 512-thread
 *                 blocks, two per CU: large grids; a plan of this family uses both depths to split a call without a slow
 *                 tail; 9: the same with seven iterations as the plan's depth: the largest grids); 8 (fp32 contexts only, LBM_ERR_ARG otherwise): seven iterations on a 64x48 region in registers
 *                 (twelve waves x four rows; six / eight iterations for what a call leaves over): large fp32 grids;
 *                 10 / 11 (fp64 contexts with "arith" 1 on a whole domain only, LBM_ERR_ARG otherwise): six / seven iterations on a
 *                 64x40 region in registers (eight waves x five rows, the fifth parked in LDS; five to seven iterations for what a
 *                 call leaves over): large fp64 grids.
 *                 Strips use 1, 6, 7 by rule with one exchange per launch; 4 / 5 (round 2's 32x16 LDS tiles) are retired,
 *                 "arith" 0 strict IEEE collision (bit-identical to the CPU oracle for normal-range operands: lbm_debug_strict_div2) | 1 FMA-contracted (<= 1e-10)
 *   strips:       "overlap" 0 launch and exchange serialised | 1 edge bands first, the exchange overlapped with the interior
 *                 rows of the SAME launch | 2 the exchange overlapped with the interior rows of the NEXT (extended)
 *                 launch; "deep_halo" 0 an exchange of LBM_HALO_ROWS rows after every launch | 1 after every second launch of a
 *                 plan of up to three iterations per launch (a deep plan still exchanges after every launch) | 2 a deep plan too:
 *                 2 x LBM_HALO_ROWS rows after every second launch of up to six iterations (both measured at lbm_initialise
 *                 when a communicator is attached, unless set here),
 *                 "halo_trim" 0 an exchange carries all nine populations of every row of a face in ONE contiguous message | 1 only the
 *                 sub-rows the receiver's launches read (the outermost row's three inbound populations, the next row's six, every
 *                 other row's nine: 9 hr - 9 of 9 hr sub-rows, five messages per face); measured at lbm_initialise like the rest,
 *                 "skip_exchange" 1 (diagnostic: no halo traffic, results invalid),
 *                 "wait_timeout_ms" bound of every host-side wait (rendezvous of a group's threads, lbm_sync, the drains of
 *                 lbm_destroy; 0 = LBM_WAIT_TIMEOUT_MS or five minutes): LBM_ERR_TIMEOUT names who was waited for,
 *                 "graph" 0|1|2 replay the launch groups of a deep strip plan from a captured hipGraph: 1 (default) where the
 *                 transport is local to the process, 2 also between the ranks of a communicator (RCCL under capture:
 *                 exercised with a one-rank communicator only so far)
 *   "stats" N     lbm_stats_begin(c, N) (before lbm_initialise: begun at its end)
 *   "frames" K    lbm_frames_begin(c, K, LBM_FRAMES_DEFAULT_CAPACITY) (before lbm_initialise: begun at its end). In
 *                 lbm_debug_choreography: the dry run records a frame sample behind every force kernel
 *   "probes" 1    lbm_debug_choreography only: the dry run records a probe sample behind every force kernel (a real context gets its
 *                 probes from lbm_probes_begin and ignores the key)
 *   "bodies" 1    lbm_debug_choreography only: the dry run records a per-body force sample behind every force kernel (a real context
 *                 gets its bodies from lbm_set_body_labels and ignores the key)
 *   "sponge" W    lbm_set_sponge(c, W, 1.5) by its key, for the dry runs, which take options only (lbm_debug_choreography); a run calls
 *                 lbm_set_sponge with a tau_end of its own
 *   "timing" 1    record HIP events around each lbm_step call (lbm_last_step_kernel_ms). */
int  lbm_set_option(lbm_ctx* c, const char* key, long value);
/* Average device time per step-kernel launch (ms) measured with HIP events on the context's stream around
 * the last lbm_step call; 0 if events were not enabled via lbm_set_option(c, "timing", 1). */
int  lbm_last_step_kernel_ms(lbm_ctx* c, double* ms_per_launch);
/* Same measurement, unreduced: device milliseconds of the last lbm_step call, the step-kernel launches it issued and
 * the iterations it advanced (a fused launch advances two to eight). */
int  lbm_last_step_stats(lbm_ctx* c, double* ms_total, int* launches, int* iterations);
/* The step kernels the launches of the last lbm_step call were dispatched as: `launches` of lbm_last_step_stats, except on a plan
 * with option "split" 3 / 4, which issues a whole-domain deep launch as that many row-range kernels on two streams (a kernel trace or a
 * counter pass sees the dispatches; timings and traffic stay per launch). No reference counterpart: the reference has no GPU path. */
int  lbm_last_step_dispatches(const lbm_ctx* c);
/* How many times a captured hipGraph of four launch groups has been replayed for this context so far (a strip with a device
 * transport on a deep plan replays its launch groups instead of issuing them call by call; option "graph" 0 turns that off;
 * 0 also where the capture was refused and the eager path runs). No reference counterpart: the reference has no GPU path. */
long lbm_graph_replays(const lbm_ctx* c);
const char* lbm_kernel_name(const lbm_ctx* c);
/* The plan lbm_initialise settled on (layout / kernel / store policy / traversal), for logs; where it was measured, with the
 * finalists' times (median of three windows each) so that the margin of the choice is visible. */
const char* lbm_plan(const lbm_ctx* c);
/* The same plan as lbm_set_option pairs, "layout=1 nt=0 alternate=1 pair_ty=12 xcd=1 deep=7": set
 * on a fresh context together with "tune" 0 they reproduce the plan in another process (bench.py's counter passes run
 * the benchmarked plan in a child process under rocprofv3). No reference counterpart. */
const char* lbm_plan_options(const lbm_ctx* c);
/* Test hook (device 0): the strict collision's two divisions by rho (LBMSolver.h:108-109) share one reciprocal chain
 * (csrc/lbm_kernels.hpp strict_div2); this runs it beside the compiler's IEEE divisions: q1,q2 = strict_div2(a1,a2,b), r1,r2 = a1/b,
 * a2/b, n host doubles each. Bit-identical for denominators in [2^-20, 2^20] and numerators 0 or of magnitude in [2^-400, 2^400]. */
int lbm_debug_strict_div2(const double* a1, const double* a2, const double* b, int n, double* q1, double* q2, double* r1, double* r2);
/* Test hook, callable without a device: the wall rule of lbm_set_wall on ONE cell — the inline function every step kernel and the
 * snapshot call (csrc/lbm_kernels.hpp wall_rule), compiled for the host. f_in9 = the cell's nine pulled populations; they are cast to the
 * element type of `precision`, the rule of wall `side` with `kind` and `velocity` is applied as on a fluid cell of that wall's row, and
 * the nine results are widened into f_out9. The argument errors of lbm_set_wall, and LBM_ERR_ARG for a null pointer or an unknown
 * precision. Replaces nothing in the reference (its rule is LBMSolver.h:155-176, kind 0). */
int lbm_debug_wall_rule(int side, int kind, double velocity, int precision, const double* f_in9, double* f_out9);
/* Test hook, callable without a device: the port rule of lbm_set_port on ONE cell - the inline function every step kernel and the
 * snapshot call (csrc/lbm_kernels.hpp port_rule), compiled for the host. f_in9 = the cell's nine populations after the pull and the wall
 * rule; they are cast to the element type of `precision`, the rule of port `side` with `kind` and `value` is applied as on a fluid cell
 * of that port's column, and the nine results are widened into f_out9, (rho, u) of the rule into *rho_out and *u_out (nullable). u_in:
 * the velocity a west VELOCITY port is given (|u_in| < 1; read by that port only). The argument errors of lbm_set_port, and LBM_ERR_ARG
 * for a null pointer, an unknown precision or such a u_in. Replaces nothing in the reference (its rules are LBMSolver.h:181-235). */
int lbm_debug_port_rule(int side, int kind, double value, double u_in, int precision, const double* f_in9, double* f_out9, double* rho_out,
                        double* u_out);
/* Test hook, callable without a device: the factor the schedule {s, n, mode} of lbm_set_inlet_schedule gives each of the nt iterations
 * t[i] >= 0, out[i] = (double)(T)s(t[i]) in the element type of `precision` — through the index function the step kernels and the
 * snapshot call (csrc/lbm_kernels.hpp inlet_sched_index), compiled for the host. The argument errors of lbm_set_inlet_schedule, and
 * LBM_ERR_ARG for n == 0, a null pointer, an unknown precision or a negative iteration. */
int lbm_debug_inlet_scale(const double* s, int n, int mode, int precision, const int* t, int nt, double* out);
/* What the head of a checkpoint says about a run (csrc/lbm_ckpt.hpp, which also describes the file): the fixed header, then for each
 * optional field whether the run has it and its value. has_*: 0 or 1; collision: 0, or the setter's model as lbm_ctx holds it (2 Smagorinsky,
 * 4 TRT, 8 forcing) with collision_param = {Cs}, {magic} or {fx, fy}; walls = {south kind, south velocity, north kind, north velocity};
 * ports = {west kind, west value, east kind, east value} (has_ports: either port is off its default); has_periodic_y: lbm_set_periodic_y. */
typedef struct lbm_ckpt_head {
    int nx, ny, y_start, local_ny, precision, steps_done;
    double tau, inlet_velocity, cylinder_x, cylinder_y, cylinder_radius;
    int has_mask, has_profile, collision, has_walls, has_sched;
    unsigned long long mask_digest, profile_digest, sched_digest;
    double collision_param[2];
    double walls[4];
    int has_ports;
    double ports[4];
    int has_periodic_y;
} lbm_ckpt_head;
#define LBM_CKPT_HEAD_MAX 184   /* bytes: no head is longer (every field present, the collision model with two parameters) */
/* Test hook, callable without a device: the head lbm_save_state writes for a context that *h describes, through the function it calls,
 * into out (cap >= LBM_CKPT_HEAD_MAX); returns its length. Where mask ([h->ny][h->nx] bytes), profile (h->ny doubles) or sched (sched_n
 * doubles, sched_mode) is not NULL, that field is marked present and its digest is formed as lbm_set_solid_mask, lbm_set_inlet_profile,
 * lbm_set_inlet_schedule form it, and left in *h. LBM_ERR_ARG: a null head or buffer, cap too small, data without a size. */
int lbm_debug_ckpt_save(lbm_ckpt_head* h, const unsigned char* mask, const double* profile, const double* sched, int sched_n, int sched_mode,
                        unsigned char* out, int cap);
/* Test hook, callable without a device: what lbm_load_state decides, through the functions it calls, about a file `path` that begins with
 * the n bytes `bytes`, on a context that *here describes: LBM_OK and in *consumed_out (nullable) the bytes of the head, behind which the
 * populations stand; or LBM_ERR_ARG with lbm_last_error() as lbm_load_state words it: "<path> is not a checkpoint", or the refusal. */
int lbm_debug_ckpt_load(const unsigned char* bytes, int n, const lbm_ckpt_head* here, const char* path, int* consumed_out);
/* Test hook, callable without a device: what the ranks of a strip run agree on before the collective schedule trials of
 * lbm_initialise (csrc/lbm_hip.hip tune_strip_schedule). per_rank7 = nranks x {may tune, overlap pinned, overlap, deep_halo pinned,
 * deep_halo, halo_trim pinned, halo_trim}; agreed7 = the same seven as agreed (-1 where nothing is pinned). LBM_ERR_ARG when the ranks pin different
 * schedules (they would otherwise run different numbers of collective trials). Replaces nothing in the reference. */
int lbm_debug_strip_pins(const int* per_rank7, int nranks, int* agreed7);
/* Test hook, callable without a device: the runs of the halo message of one face of `hr` rows (option "halo_trim"; csrc/lbm_strips.inc.hpp
 * face_runs) as up to five {first sub-row, sub-rows} pairs relative to the first sub-row of the block (row-interleaved layout: nine
 * sub-rows per lattice row); south_block != 0: the block lies below the strip it borders (a sender's top rows / a receiver's south ghost
 * rows). Returns the number of runs. Replaces the nine-values-per-edge-cell buffers of pack_data_for_sending, LBMGrid.h:395-440. */
int lbm_debug_face_runs(int hr, int trim, int south_block, int* runs10);
/* Test hook, callable without a device: the index arithmetic of the device rings that the output iterations fill and the drains empty
 * (the two force logs, frames, probes: csrc/lbm_plan.hpp RingIndex), on one ring of `capacity` slots driven through `nops` operations.
 * ops[k] < 0 pushes a sample, ops[k] = m >= 0 takes up to m of the oldest. out3[3k..3k+2]: a push: {its slot, -1, -1}, or {-1, -1, -1}
 * on a full ring (nothing changes); a take: {start, n1, n2}: slots [start, start + n1), then [0, n2). Returns the samples pending at
 * the end; LBM_ERR_ARG: capacity < 1 or a null pointer. Replaces nothing in the reference. */
int lbm_debug_ring(int capacity, const int* ops, int nops, int* out3);
/* Test hook, callable without a device: the candidate plans lbm_initialise would time on a whole-domain context of this grid
 * (csrc/lbm_plan.hpp), one per line: "name|lbm_set_option pairs|dominant kernel|iterations per launch". */
int lbm_debug_plan_candidates(int nx, int ny, int precision, int arith, int num_cus, char* out, int cap);
/* Test hook, callable without a device: the setters of the collision models on a context that is never initialised on a device (64 x 64
 * cells, the given tau and precision, `options` = "key=value ..." as for lbm_set_option applied first). Call k is setter[k] with
 * (v1[k], v2[k]): 0 lbm_set_smagorinsky(v1), 1 lbm_set_trt(v1), 2 lbm_set_forcing(v1, v2), 3 lbm_set_mrt(v1, v2), 4 marks the context
 * initialised (as lbm_initialise leaves it), 5 lbm_initialise's refusal of a pinned deep shape, 6 lbm_set_sponge((int)v1, v2). rc[k] receives each return value, `texts`
 * one line per call: the error text of a failed call, empty for LBM_OK. collision3 receives {lbm_ctx::collision, and what lbm_get_mrt
 * reports}. LBM_ERR_ARG: a null pointer, an unknown setter, a bad option, a buffer too small. */
int lbm_debug_collision_setters(double tau, int precision, const char* options, const int* setter, const double* v1, const double* v2, int n,
                                int* rc, char* texts, int cap, double* collision3);
/* Test hook, callable without a device: what the step kernels of one collision model are handed per launch. On the context of
 * lbm_debug_collision_setters (the given tau and precision) the one setter is applied with (v1, v2), numbered as there: 0, 1, 2, 3, 6,
 * or -1 for plain BGK; the kernel arguments are filled as for a launch, and the model's values are read back by the code the kernels
 * read them with. out receives them as doubles in the order BGK {wp}, Smagorinsky {tau, tau^2, C}, TRT {wp, wm, wa, wb}, forcing
 * {wp, gx, gy, hx, hy}, MRT {wp, wm, wa, wb, sb, kb}, sponge {}, and behind them the raw content of the seven slots the models share:
 * the four of the forcing block, then the three behind them. Returns the number of named values (the seven follow), or what the setter
 * returned; LBM_ERR_ARG besides: a null pointer, an unknown setter, cap below the count. */
int lbm_debug_collision_args(double tau, int precision, int setter, double v1, double v2, double* out, int cap);
/* Test hook, callable without a device: lbm_set_sponge(width, tau_end) on a context of nx columns that is never initialised on a device
 * (the given tau and precision), then lbm_get_sponge into pair2 = {width, tau_end} and lbm_get_sponge_rate of every column into
 * rates[nx]. Returns what lbm_set_sponge returned (its text: lbm_last_error); the getters run either way. LBM_ERR_ARG besides: a null
 * pointer, nx < 1. */
int lbm_debug_sponge_rates(int nx, double tau, int precision, int width, double tau_end, double* pair2, double* rates);
/* Test hook, callable without a device: the table behind option "deep" (csrc/lbm_plan.hpp deep_shapes, region_kinds), one line per id,
 * precision and arithmetic mode that exists: "id|f64 or f32|strict or contracted|lds or registers|iterations per launch|width|height of
 * the tile or region|rows per thread|waves|offered depths|restrictions". An offered depth of a register shape reads
 * "depth:nt+plain" or "depth:plain" (the store policies instantiated), with ":no-face" where a context with a strip face may not
 * launch it. LBM_ERR_ARG: a null pointer or a buffer too small. */
int lbm_debug_deep_shapes(char* out, int cap);
/* Test hook, callable without a device: the host threads that drive the strips of an in-process group (csrc/lbm_ctx.hpp GroupPool) on a
 * dummy job of `rounds` rounds with one rendezvous each, `repeat` times on one pool; in the last run strip `fail_strip` reports an
 * injected error in round `fail_round` and strip `stall_strip` sleeps `stall_ms` before the rendezvous of round `stall_round` (-1:
 * nobody). Returns what the last run returned: LBM_OK, the injected LBM_ERR_HIP (every thread left at the same rendezvous), or
 * LBM_ERR_TIMEOUT naming the strip that was waited for (bound: timeout_ms; 0 = LBM_WAIT_TIMEOUT_MS). *rendezvous_out = rendezvous strip
 * 0 passed in the last run. The reference's counterpart are the implicit barriers of its OpenMP regions (LBMSolver.h:87,131). */
int lbm_debug_group_pool(int n, int rounds, int fail_strip, int fail_round, int stall_strip, int stall_round, int stall_ms, long timeout_ms, int repeat,
                         int* rendezvous_out);
/* Test hook, callable without a device: a DRY RUN of the launch choreography of a strip run and its check (csrc/lbm_choreo.inc.hpp). The
 * functions that issue a launch group (plan_launch, issue_before, the exchanges, issue_after) run on contexts without a device and
 * record every kernel (with the rows it writes and, through its depth, reads), event record, cross-stream wait, copy, send and receive;
 * the record is replayed with vector clocks. Returns the number of violations — RACE: two accesses to the same row of the same buffer, at
 * least one of them a write, that no event orders; STALE: a launch (or the force kernel, or — option "stats" — the statistics sample, which
 * also reads one ghost row per face, or — option "bodies" — the per-body force sample, which reads the force kernel's rows and writes a log slot of its own, or — option "frames" —
 * the frame sample, which reads the force kernel's rows plus TWO ghost rows per face (the ghost row next to the face for d/dy, and the
 * row beyond it that this row's outlet cell pulls from) and writes a ring slot of its own, or — option "probes" — the probe sample, which
 * reads rows [-1, local_ny + 2) of buf[cur] (a probe's y1 on the ghost row next to the north face and the row its inlet / outlet cell
 * pulls from; the pull of row 0) and writes a ring slot of its own) reads a row that does not hold the iteration it
 * needs — or < 0; `out` receives their description (and, with dump != 0, every recorded operation). What it replaces: the ordering the
 * reference gets from MPI_Waitall before unpack_received_data (LBMGrid.h:278-283).
 * bounds2 = nstrips x {y_start, rows}; transport 0 in-process group with peer copies, 1 in-process group over RCCL, 2 ONE strip as a rank
 * of a multi-process RCCL run (its faces follow from y_start / rows / ny), 3 ONE strip exchanging with itself (loopback copies);
 * options = "key=value ..." as for lbm_set_option (the plan must be pinned: nothing is measured); calls2 = ncalls x {nsteps, output_frequency}. */
int lbm_debug_choreography(int nx, int ny, const int* bounds2, int nstrips, int precision, int transport, const char* options,
                           const int* calls2, int ncalls, int dump, char* out, int cap);
/* Test hook, callable without a device: exchange_rccl's multi-rank branch — the one piece of the library no run has executed yet (it needs two
 * GPUs) — run DRY on every rank of an `nranks`-process strip run: each rank issues its launch groups as in lbm_debug_choreography and the
 * posting loops hand their sends / receives (peer, offset, count) to a transcript instead of RCCL. RCCL pairs the k-th send to a peer with the
 * peer's k-th receive from the sender: the hook checks, for every pair of neighbours and both directions, that the sequences have the same
 * length and counts and that every message leaves and lands at the same offset inside its block of edge / ghost rows, and that all ranks
 * issue the same number of exchanges. Returns the number of mismatches (0 = the ranks would pair up) or < 0; `out` describes them.
 * options: for every rank; options_rank1 (nullable): additionally for rank 1 only — ranks that disagree (e.g. on "halo_trim") must be
 * flagged. Replaces the tag / count matching of the reference's MPI_Isend / MPI_Irecv pairs (LBMGrid.h:255-276). */
int lbm_debug_p2p_matching(int nx, int ny, const int* bounds2, int nranks, int precision, const char* options, const char* options_rank1,
                           const int* calls2, int ncalls, char* out, int cap);
/* Test hook, callable without a device: the packing lbm_set_solid_mask makes for the strip [y_start, y_start + local_ny) of a global
 * [ny][nx] mask (csrc/lbm_geom.hpp). dims9 = {first window row, window rows, 64-bit words per row, 8x8 blocks per row, block rows,
 * bounding box of the whole mask x0, x1, y0, y1 (x1 < x0: no solid cell)}; bits ([rows][words]) and sat ([block rows + 1][blocks + 1],
 * the summed-area table of solid counts per 8x8 block) are copied where not null. near_out[k] = the kernels' block-uniform query
 * "any solid cell in the box" for boxes4[k] = {x0, x1, y0, y1} (global, inclusive), answered from the coarse table. */
int lbm_debug_geometry(const unsigned char* mask, int nx, int ny, int y_start, int local_ny, int* dims9, unsigned long long* bits, long bits_cap,
                       int* sat, long sat_cap, const int* boxes4, int nbox, int* near_out);
/* Test hook, callable without a device: the verdict the register kernel k_stepc_col reaches for ONE WAVE of a tile that is not lean as
 * a whole — may the wave run the lean path although its block does not (csrc/lbm_kernels.hpp wave_plain, the very function the kernel's
 * branch calls, compiled for the host)? The context is described: the strip [y_start, y_start + local_ny) of an nx x ny lattice in
 * `precision` with arithmetic `arith` (0 strict, 1 contracted), periodic_y as lbm_set_periodic_y, `mask` as lbm_set_solid_mask takes it
 * (NULL: the disc of cylinder3 = {x / nx, y / ny, radius / ny}; NULL: 0.2, 0.5, 0.05). The launch: `depth` iterations on the regions of
 * shape `deep` (option "deep": a register shape) over the local rows [y_lo, y_lo + y_cnt) (y_cnt <= 0: the whole strip; a range launch
 * of option "split" or an edge band otherwise). The wave: `wave` of tile column bx, band by of that range. Returns 1 (plain), 0, or
 * LBM_ERR_ARG. dims4 (nullable) = {rows per thread, waves per block, the block's own lean verdict, its near-solid verdict}. Walls, ports
 * and inlet profiles need no argument: they act on rows 0 and ny - 1 and on columns 0 and nx - 1, which no plain wave holds.
 * No reference counterpart. */
int lbm_debug_wave_plain(int nx, int ny, int y_start, int local_ny, int precision, int arith, int periodic_y, const unsigned char* mask,
                         const double* cylinder3, int deep, int depth, int y_lo, int y_cnt, int bx, int by, int wave, int* dims4);
/* Test hook, callable without a device: what lbm_set_body_labels derives from a global [ny][nx] label array for the strip
 * [y_start, y_start + local_ny) (csrc/lbm_geom.hpp pack_bodies). Returns B (or < 0). boxes4 (nullable, boxes_cap entries of four ints) =
 * B x {x0, x1, y0, y1}: body k's bounding box dilated by one cell, clipped to the domain and to the strip's rows, inclusive, y in LOCAL
 * rows; {0, -1, 0, -1} for a body with no cell or with nothing of its box in the strip. chunks3 (nullable, chunks_cap entries of three
 * longs) = the chunk table {body, first cell in the box's row-major order, cells}: every non-empty box cut into runs of 65536 cells,
 * bodies in label order; *nchunks_out (nullable) = its length. No reference counterpart. */
int lbm_debug_body_chunks(const unsigned char* labels, int nx, int ny, int y_start, int local_ny, int* boxes4, int boxes_cap,
                          long* chunks3, int chunks_cap, int* nchunks_out);
/* Test hook, callable without a device: the table lbm_probes_begin uploads for the strip [y_start, y_start + local_ny) of an nx x ny
 * lattice (csrc/lbm_probes.hpp probe_entry), with lbm_probes_begin's checks of xy and n. Per probe: cells4 = {x0, LOCAL y0, x1, LOCAL y1}
 * with x1, y1 clamped at the domain's edge as k_probes clamps them (local y1 == local_ny: the ghost row next to the north face), weights2 =
 * {fx, fy}, owned = 1 where floor(py) lies in the strip's rows; a probe that is not owned has cell (0, 0) and weights 0. Any output may be
 * NULL. Returns n or < 0. No reference counterpart. */
int lbm_debug_probe_table(const double* xy, int n, int nx, int ny, int y_start, int local_ny, int* cells4, double* weights2, int* owned);
/* Test hook, callable without a device: the rules of the group gathers (csrc/lbm_gather.hpp) applied to caller-supplied host arrays, one
 * per strip. bounds2 = n x {y_start, rows} of a lattice of ny rows of nx cells; parts[i] = strip i's array; what selects the routine:
 * 0 stack `planes` planes of doubles, parts[i] = [planes][rows / k][nx / k], into whole = [planes][ny / k][nx / k] at row y_start / k
 * (k = 1: the fine grid); 1 its inverse (whole -> parts); 2 as 0 on floats (frames); 3 ghost-inclusive populations, parts[i] =
 * [rows + 2][nx + 2][9] into whole = [ny + 2][nx + 2][9] by the ghost-row rule of lbm_group_get_populations; 4 the in-order sum of the
 * strips' nx * planes doubles into whole (the bounds only have to lie in the lattice). LBM_ERR_ARG: a null pointer, what outside 0..4, a
 * size < 1 or a strip outside the lattice. No reference counterpart. */
int lbm_debug_gather(int what, int n, const int* bounds2, int nx, int ny, int k, int planes, void* const* parts, void* whole);
/* SHA-256 (16 hex digits) of the sources this binary was compiled from (csrc/ and this header); build.py rebuilds
 * when it differs from the tree, bench.py prints it. */
const char* lbm_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
