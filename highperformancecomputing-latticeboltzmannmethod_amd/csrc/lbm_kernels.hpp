// csrc/lbm_kernels.hpp — device code of the D2Q9-BGK timestep for gfx950 (CDNA4, wave64).
//
// One persistent state per strip: the POST-COLLISION populations P_t (the reference's f_next right after
// collision_step() of iteration t, LBMSolver.h:84-126), stored as 9 SoA planes with a one-cell ghost frame:
//
//     plane i, local row gy in [0, ny_loc+2*GR), column col:   base[i*plane + gy*pitch + col]
//     interior cell (x, y)  <->  gy = y+GR, col = xoff + x      (xoff*sizeof(T) is a multiple of 128 B)
// GR = 12 ghost rows on each side, of which a strip exchanges six (once per launch of up to six fused iterations, or once
// per TWO launches of up to three: the first launch of such a pair also updates three ghost rows per internal face,
// redundantly with the neighbour, so that the second one finds valid inputs); one ghost column on each side.
// The two strides describe either of two layouts chosen by the host (lbm_hip.hip, "plan"):
//     PLANAR          plane = rows*pitch0 (+pad), pitch = pitch0            nine separate planes
//     ROW-INTERLEAVED plane = pitch0,             pitch = 9*pitch0          [gy][i][col]: the nine sub-rows of a
//                     lattice row are adjacent, so a block's 18 streams stay inside two ~300 KB windows
// Every kernel below is layout-agnostic: it only uses (plane, pitch).
//
// Ghost cells hold, permanently and in BOTH A/B buffers, what the reference's halo logic leaves in them on one
// rank: E/W ghost columns of globally-interior rows = 0, physical N/S ghost rows and the
// four corner ghosts = the initial equilibrium; solid cells hold w_i for ever (N4). Strip-internal ghost rows
// are refreshed every step by the halo exchange. The step kernel therefore needs no boundary branches for
// its nine pulls and writes fluid interior cells only.
//
// Kernel families (within one arithmetic mode all evaluate the SAME per-cell operation sequence => bit-identical results):
//   k_step_site                  one iteration per launch, 144 B of HBM traffic per lattice update (fp64)
//   k_step2/3/4_tile             two / three / four iterations per launch over 64 x TY tiles, intermediate states in LDS
//                                (what a call's last iterations, short strips and the strict mode's measurement use)
//   k_stepd_tile                 six / seven / eight iterations on an LDS-filling tile: grids of a single round of blocks
//   k_stepc_col                  (lbm_kernel_col.hpp) five / six iterations with the lattice of a 64x32 region held in
//                                registers: the production kernel of large grids and tall strips
//   k_init, k_macros, k_forces, k_halo_pack/unpack   set-up and the output cadence
// The fused kernels share the per-cell rule (cell_update / cell_update_last over bcs_at) and the block prologue (TileFrame);
// k_step3_tile, k_step4_tile and k_stepd_tile are one body (step_tile) at depth 3, 4 and 6..8.
// Arithmetic modes of the collision (enum Arith): strict IEEE operation by operation (bit-identical to the CPU oracle)
// or FMA-contracted with one reciprocal (what the reference's -ffast-math -mfma build permits; <= 1e-10).
// The collision itself is lbm_collision.hpp, included below: one operator per model and arithmetic mode, each model's launch-uniform
// values under their own names with the one map of those names to the slots of KArgs, and collide(), which picks by Arith.
//
// Step kernel K_t (one iteration = one loop body of Solver::run, LBMSolver.h:49-60):
//     pull from P_t        == exchange_ghost_cells + streaming_step        (LBMGrid.h:249, LBMSolver.h:128-145)
//     wall / inlet / outlet== apply_boundary_conditions, sequential order  (LBMSolver.h:147-236)
//     stability test       == Grid::check_stability                        (LBMGrid.h:285-317)
//     moments + collide()  == collision_step of iteration t+1              (LBMSolver.h:84-126)
//     store P_{t+1}
// Algorithmic traffic: 9 loads + 9 stores per lattice update = 144 B (fp64) / 72 B (fp32). HBM-bound; no MFMA.
#pragma once
#include <cstddef>
#include <utility>
#include <hip/hip_runtime.h>

namespace lbmk {

constexpr int Q = 9;
constexpr int GR = 12;  // ghost rows ALLOCATED below and above the strip (the frame every kernel addresses rows by: gy = y + GR)
constexpr int HR1 = 6;  // ghost rows a strip's halo exchange refreshes per face (LBM_HALO_ROWS): one launch of up to six fused
                        // iterations, or two of up to three (the first of the pair recomputes three of the neighbour's rows), between
                        // exchanges. With "deep_halo" 2 (round 4) a deep plan exchanges all GR = 12 rows once per TWO launches of up to six
                        // iterations each: the first launch of such a pair also updates the six ghost rows next to each internal face.
// LBMConfig.h:13-34 — direction numbering is observable through f_current(x,y,i), keep it.
__host__ __device__ constexpr int cx(int i) { constexpr int v[Q] = {0, 1, 0, -1, 0, 1, -1, -1, 1}; return v[i]; }
__host__ __device__ constexpr int cy(int i) { constexpr int v[Q] = {0, 0, 1, 0, -1, 1, 1, -1, -1}; return v[i]; }
__host__ __device__ constexpr int opp(int i) { constexpr int v[Q] = {0, 3, 4, 1, 2, 7, 8, 5, 6}; return v[i]; }
template <typename T> __host__ __device__ constexpr T wgt(int i) {
    return i == 0 ? T(4.0 / 9.0) : (i < 5 ? T(1.0 / 9.0) : T(1.0 / 36.0));
}

// User-defined geometry (lbm_set_solid_mask): a read-only bitmap of the rows a strip can ever query, its own rows +- GR
// clipped to the domain, built on the host and uploaded once; no kernel writes it. Beside it a summed-area table of the solid
// counts of 8x8-cell blocks of the same window, so that "can this tile touch a solid cell" stays O(1) (four lookups) for any mask.
struct MaskView {
    const unsigned long long* bits = nullptr;   // [rows][words]: bit x & 63 of word x >> 6 of row r = cell (x, y0 + r)
    const int* sat = nullptr;                   // [nby + 1][nbx + 1]: sat[b][c] = solid cells in the blocks < b (rows) and < c (columns)
    int y0 = 0, rows = 0, words = 0, nbx = 0, nby = 0;
};
__host__ __device__ inline bool mask_cell(const MaskView& m, int x, int yg) {   // 0 <= x < nx; rows outside the window: fluid
    const int r = yg - m.y0;
    if (r < 0 || r >= m.rows) return false;
    return (m.bits[(long)r * m.words + (x >> 6)] >> (x & 63)) & 1ull;
}
// the word of mask_cell's bit, 0 where mask_cell answers false without a read: the same address under the same test, for a caller that
// issues the read early and looks at bit x & 63 later (k_stepc_col)
__device__ __forceinline__ unsigned long long mask_word(const MaskView& m, int x, int yg) {
    const int r = yg - m.y0;
    return (r < 0 || r >= m.rows) ? 0ull : m.bits[(long)r * m.words + (x >> 6)];
}
// any solid cell in [x0, x1] x [yg0, yg1] (global, inclusive)? Exact at block granularity, so a superset of the cell test: it never
// answers false where a solid cell lies in the box.
__host__ __device__ inline bool mask_box_any(const MaskView& m, int x0, int x1, int yg0, int yg1) {
    x0 = x0 < 0 ? 0 : x0;
    x1 = x1 > m.nbx * 8 - 1 ? m.nbx * 8 - 1 : x1;
    const int r0 = yg0 - m.y0 < 0 ? 0 : yg0 - m.y0, r1 = yg1 - m.y0 > m.rows - 1 ? m.rows - 1 : yg1 - m.y0;
    if (x0 > x1 || r0 > r1) return false;
    const int W = m.nbx + 1, c0 = x0 >> 3, c1 = (x1 >> 3) + 1, b0 = r0 >> 3, b1 = (r1 >> 3) + 1;
    return m.sat[b1 * W + c1] - m.sat[b0 * W + c1] - m.sat[b1 * W + c0] + m.sat[b0 * W + c0] > 0;
}

// Kinds of a physical wall (lbm_set_wall, include/lbm_hip.h LBM_WALL_*) and the word that carries both through the argument blocks:
// the south wall's kind in bits 0-1, the north wall's in bits 2-3. 0 = both walls no-slip, the reference's.
enum WallKind { WALL_NOSLIP = 0, WALL_FREESLIP = 1, WALL_MOVING = 2 };
__host__ __device__ constexpr int wall_pack(int south, int north) { return south | (north << 2); }
// What a wall adds to / subtracts from the two diagonal populations it writes, per wall (s: south, n: north). Moving: both are the momentum
// correction k = u_w / 6 = 6 w_i rho_w (c_i . u_w) with rho_w = 1, formed in double and cast. Other kinds: the operands that change no bit
// of any value, x + (-0.0) and x - (+0.0) (the sign of a zero included), so the rule needs no branch on "moving".
template <typename T> struct WallK { T s_add, s_sub, n_add, n_sub; };
template <typename T>
inline WallK<T> wall_ks(int south, double u_south, int north, double u_north) {
    WallK<T> k;
    k.s_add = south == WALL_MOVING ? (T)(u_south * (1.0 / 6.0)) : T(-0.0);
    k.s_sub = south == WALL_MOVING ? (T)(u_south * (1.0 / 6.0)) : T(0.0);
    k.n_add = north == WALL_MOVING ? (T)(u_north * (1.0 / 6.0)) : T(-0.0);
    k.n_sub = north == WALL_MOVING ? (T)(u_north * (1.0 / 6.0)) : T(0.0);
    return k;
}

// The two ports (lbm_set_port, include/lbm_hip.h LBM_PORT_*): the west one is column 0, the east one column nx - 1; each is a Zou-He
// rule with the velocity given and the density solved for, or the density given and the velocity solved for. The two kinds ride in the
// spare bits of the word that carries the walls (wall_pack above uses bits 0-3): bit 4 set = the west port is a PRESSURE port, bit 5
// set = the east port is a VELOCITY port, so the reference's pair (velocity inlet, pressure outlet) is 0 in both.
enum PortKind { PORT_VELOCITY = 0, PORT_PRESSURE = 1 };
constexpr int PORT_WEST_PRESSURE = 16, PORT_EAST_VELOCITY = 32;
__host__ __device__ constexpr int port_pack(int west_kind, int east_kind) {
    return (west_kind == PORT_PRESSURE ? PORT_WEST_PRESSURE : 0) | (east_kind == PORT_VELOCITY ? PORT_EAST_VELOCITY : 0);
}
// What the two ports are given, formed on the host in double and cast once: the west port's density (read by a pressure port only; a
// velocity port takes its velocity per row and iteration from u_row and the schedule) and the east port's density or velocity.
// east_den is what the east rule divides S by: the density of a pressure port, 1 + u of a velocity port — that ONE addition in the
// element type, the operation the table writes, done here once instead of by every thread of the column.
template <typename T> struct PortK { T west, east, east_den; };
template <typename T>
inline PortK<T> port_ks(double west_value, int east_kind, double east_value) {
    const T e = (T)east_value;
    return PortK<T>{(T)west_value, e, east_kind == PORT_VELOCITY ? T(1.0) + e : e};
}


template <int N> struct KPad { char b[N]; };
template <> struct KPad<0> {};

template <typename T>
struct KArgs {
    // Four of the slots that carry the collision models' launch-uniform values (tau_inv and the three unions below are the others; which
    // model's value stands in which slot is written once, in the slot map of lbm_collision.hpp, and no other code names them): four
    // values where the unions have three. A block of exactly 64 bytes IN FRONT of everything else, not behind it like the additions below: the fused kernels' second
    // argument block (K2Extra) follows this struct in the kernel-argument segment, and the compiler merges the scalar loads of adjacent
    // fields across the two by their alignment, up to 64 bytes. Four values behind `sched` part the two blocks and 26 earlier
    // instantiations came out with other scalar spills or vector register counts; with every field moved by 64 bytes, K2Extra's
    // included, each of them keeps its loads and its register allocation (profiles/forcing/README.md).
    // The values of the two ports (lbm_set_port; the kinds ride in `walls`) stand in what was padding of this block, for the same
    // reason: no field of KArgs or K2Extra moves. Launch-uniform: read inside the inlet / outlet branches of apply_bcs only.
    // The outlet sponge's table (lbm_set_sponge) takes the last eight bytes of the block, which were padding too: 1/tau_x of every column of
    // the domain, nx elements, each formed on the host in double and cast once; nullptr on every other context. Read only by the sponge
    // instantiations (AR_STRICT_SPONGE / AR_CONTRACTED_SPONGE), through column_rate.
    T frc_gx, frc_gy, frc_hx, frc_hy;
    PortK<T> pk;
    [[no_unique_address]] KPad<56 - 7 * sizeof(T)> frc_pad;
    const T* wp_x;
    const T* src;      // plane 0 of the buffer read  (P_t)
    T* dst;            // plane 0 of the buffer written (P_{t+1})
    long plane;        // elements per plane
    int pitch;         // elements per row
    int xoff;          // column of interior x = 0
    int nx, ny_loc;    // interior size of this strip
    int ny_glob;       // global rows
    int y_start;       // global row of local y = 0
    int cyl_x, cyl_y;  // LBMConfig.h:61-63 (integer cells)
    double cyl_r2;     // (double)(r*r), LBMGrid.h:169
    MaskView mv;       // user-defined geometry (lbm_set_solid_mask); mv.bits == nullptr: the disc above
    T tau_inv;         // 1/tau, LBMSolver.h:85 (a slot of the collision models' values: lbm_collision.hpp)
    const T* u_row;    // inlet velocity of global row yg at u_row[yg], every row of the domain: inlet_velocity on every row, or the
                       // profile of lbm_set_inlet_profile. Read on the inlet column (x == 0) only, inside apply_bcs
    int* unstable_t;   // device word: first unstable iteration (INT_MAX if none)
    int t;             // iteration this launch completes, RELATIVE to *t_base (stability bookkeeping; the inlet schedule's entry)
    const int* t_base; // device word: the iteration `t` counts from. A launch replayed from a hipGraph carries a fixed `t`; the
                       // word is advanced on the device between replays. Read on the (rare) unstable path, and on the inlet column
                       // of a context with an inlet schedule (bcs_at), only.
    int y_lo, y_cnt;   // local rows [y_lo, y_lo + y_cnt) covered by this launch
    int y_lo2, y_cnt2; // optional second range [y_lo2, y_lo2 + y_cnt2) of the same launch (both edge bands of a strip
                       // in one grid); y_cnt2 == 0: none
    int reverse;       // 1: blockIdx.y walks the rows top-down (alternated per launch by the host, see row_of_block)
    // Three more slots of the collision models' values (lbm_collision.hpp: the slot map), appended so that the fields BGK kernels read
    // keep their offsets, and shared by the models that came later (a context has one model), so that the struct, and with it every
    // earlier kernel, keeps its size and offsets. The names are those of the first two models that used them.
    union { T les_tau; T trt_wm; };
    union { T les_tau2; T trt_wa; };
    union { T les_c; T trt_wb; };
    // The two physical walls (lbm_set_wall), appended for the same reason: wall_pack of the two kinds, and what each wall adds to and
    // subtracts from its diagonal populations (wall_ks: k = u_w / 6 of a moving wall, formed on the host in double; the identity
    // operands otherwise). Launch-uniform: read inside the bottom / top branches of apply_bcs only. Bits 4 and 5 of `walls` are the
    // kinds of the two ports (port_pack), read inside the inlet / outlet branches only.
    int walls;
    WallK<T> wk;
    // The inlet schedule (lbm_set_inlet_schedule), appended likewise: the device block {int n; int mode; T s[n]} (inlet_sched_at), nullptr
    // without one. Launch-uniform: tested and read inside the inlet branch of apply_bcs only.
    const int* sched;
};
static_assert(offsetof(KArgs<double>, wp_x) == 56 && offsetof(KArgs<double>, src) == 64 && offsetof(KArgs<float>, wp_x) == 56 &&
              offsetof(KArgs<float>, src) == 64, "the block in front of KArgs is 64 bytes, the sponge's table its last eight");
// ... and the slots of the collision models' launch-uniform values (lbm_collision.hpp maps each model's names to them): the offsets are
// what keeps every kernel at its scalar loads and register counts (profiles/forcing/README.md)
template <typename T> constexpr bool collision_slots_at(size_t tau_inv, size_t u0) {
    return offsetof(KArgs<T>, frc_gx) == 0 && offsetof(KArgs<T>, frc_gy) == sizeof(T) && offsetof(KArgs<T>, frc_hx) == 2 * sizeof(T) &&
           offsetof(KArgs<T>, frc_hy) == 3 * sizeof(T) && offsetof(KArgs<T>, tau_inv) == tau_inv && offsetof(KArgs<T>, les_tau) == u0 &&
           offsetof(KArgs<T>, trt_wm) == u0 && offsetof(KArgs<T>, les_tau2) == u0 + sizeof(T) && offsetof(KArgs<T>, trt_wa) == u0 + sizeof(T) &&
           offsetof(KArgs<T>, les_c) == u0 + 2 * sizeof(T) && offsetof(KArgs<T>, trt_wb) == u0 + 2 * sizeof(T);
}
static_assert(collision_slots_at<double>(168, 232) && collision_slots_at<float>(168, 228) && sizeof(KArgs<double>) == 304 &&
              sizeof(KArgs<float>) == 272, "the collision models' slots and the size of KArgs stay as they are");

// Row handled by blockIdx.y. Blocks are dispatched roughly in index order; walking the rows in the opposite
// direction on every other step makes a step start on the rows the previous step wrote last, which are the
// ones most likely still resident in the 256 MiB Infinity Cache (measured +0..8 % at 4096x1024 fp64).
template <typename T>
__device__ __forceinline__ int row_of_block(const KArgs<T>& a) {
    const int by = (int)blockIdx.y;            // grid.y == y_cnt + y_cnt2
    if (by >= a.y_cnt) return a.y_lo2 + (by - a.y_cnt);
    return a.y_lo + (a.reverse ? a.y_cnt - 1 - by : by);
}

// Tile band of a fused launch: bands of TY rows over the first range, then over the second (grid.y = both counts).
// Returns the first row of the band and, through y_end, the end of the range it belongs to.
template <typename T>
__device__ __forceinline__ int band_origin(const KArgs<T>& a, int by, int TY, int& y_end) {
    const int nb1 = (a.y_cnt + TY - 1) / TY;
    if (by >= nb1) { y_end = a.y_lo2 + a.y_cnt2; return a.y_lo2 + (by - nb1) * TY; }
    y_end = a.y_lo + a.y_cnt;
    return a.y_lo + by * TY;
}

// Grid::setup_geometry, LBMGrid.h:152-173, as a pure function of GLOBAL integer coordinates.
__device__ __forceinline__ bool is_solid_cell(int x, int yg, int cyl_x, int cyl_y, double cyl_r2) {
    const double dx = (double)(x - cyl_x), dy = (double)(yg - cyl_y);
    return dx * dx + dy * dy <= cyl_r2;
}

// The one geometry test of every kernel: the mask where one is set, else the disc. `a` is any argument block with the disc
// and a MaskView (KArgs, InitArgs, MacroArgs, ForceArgs); the branch is uniform over the launch. 0 <= x < nx.
template <typename A>
__device__ __forceinline__ bool solid_at(const A& a, int x, int yg) {
    return a.mv.bits ? mask_cell(a.mv, x, yg) : is_solid_cell(x, yg, a.cyl_x, a.cyl_y, a.cyl_r2);
}

// Block-uniform test: can any cell of the tile [X0, X0+TX) x [Y0, Y0+TY) grown by `ring` cells be solid? Disc: bounding
// boxes in integer cells (cyl_r2 = r*r exactly, so r is recovered by an exact sqrt of a perfect square). Mask: the coarse table
// with the box rounded outward to 8x8 blocks. Both exact or conservative: false only where no cell of the box is solid.
// __host__ too: lbm_debug_wave_plain asks it on the CPU.
template <typename T>
__host__ __device__ __forceinline__ bool tile_near_solid(const KArgs<T>& a, int X0, int Y0, int TX, int TY, int ring) {
    const int yg0 = a.y_start + Y0;
    if (a.mv.bits) return mask_box_any(a.mv, X0 - ring, X0 + TX - 1 + ring, yg0 - ring, yg0 + TY - 1 + ring);
    const int r = (int)sqrt(a.cyl_r2) + 1;
    return X0 - ring <= a.cyl_x + r && X0 + TX - 1 + ring >= a.cyl_x - r &&
           yg0 - ring <= a.cyl_y + r && yg0 + TY - 1 + ring >= a.cyl_y - r;
}

// The inlet schedule (lbm_set_inlet_schedule): which entry of a table of n scale factors iteration t >= 0 takes. HOLD (mode 0): the last
// entry holds for ever; REPEAT (mode 1): the table is periodic. The one statement of it: the step kernels, the snapshot's host side
// (lbm_get_inlet_scale, MacroArgs::in_scale) and lbm_debug_inlet_scale call this function.
// Unsigned arithmetic: the result lies in [0, n) for every bit pattern of t, so no iteration number can take a read out of the table.
__host__ __device__ inline int inlet_sched_index(int t, int n, int mode) {
    const unsigned ut = (unsigned)t, un = (unsigned)n;
    return (int)(mode == 1 ? ut % un : (ut < un - 1u ? ut : un - 1u));
}
// The schedule as the kernels read it: two ints, then the n factors in the element type at byte 8 (aligned for both types).
constexpr int INLET_SCHED_HEAD = 2;
template <typename T>
__device__ __forceinline__ T inlet_sched_at(const int* sched, int t) {
    return reinterpret_cast<const T*>(sched + INLET_SCHED_HEAD)[inlet_sched_index(t, sched[0], sched[1])];
}

// The wall rule of ONE cell of global row 0 (bottom) or ny - 1 (top): the reference's on-node bounce-back (:155-163, :168-176) with the
// wall's kind deciding what the two diagonal populations it writes become:
//   no-slip    f5 = f7, f6 = f8 (south); f7 = f5, f8 = f6 (north): the reference's
//   free-slip  the two sources change places (specular reflection: f5 = f8, f6 = f7 at the south wall)
//   moving     no-slip's, +k / -k with k = u_w / 6: ONE IEEE addition each, so strict and contracted arithmetic apply the same bits.
//              rho_w is 1, not the cell's density, and the on-node scheme does not make ux on the wall's row equal u_w.
// Every kind keeps the pair sums, hence mass, as bounce-back does. `walls` and the four operands are launch-uniform (scalar registers).
// Written without a branch on the kind: the SOURCE of each population is chosen, then the operand of WallK is added or subtracted, which
// for a wall that does not move is the identity on every bit pattern (wall_ks). No value is live that bounce-back does not hold, and no
// kernel loses an occupancy step to the rule. (Bounce-back followed by a swap of the two results under a uniform branch computes the
// same and compiled to 16 more VGPRs in k_step_site and an occupancy step less in k_frame and k_probes: profiles/walls/README.md.)
// __host__ too: lbm_debug_wall_rule applies this very function on the CPU.
template <typename T>
__host__ __device__ __forceinline__ void wall_rule(T (&f)[Q], bool bottom, bool top, int walls, const WallK<T>& k) {
    if (bottom) {
        const bool fs = (walls & 3) == WALL_FREESLIP;
        const T a = fs ? f[8] : f[7], b = fs ? f[7] : f[8];
        f[2] = f[4]; f[5] = a + k.s_add; f[6] = b - k.s_sub;
    }
    if (top) {
        const bool fs = ((walls >> 2) & 3) == WALL_FREESLIP;
        const T a = fs ? f[6] : f[5], b = fs ? f[5] : f[6];
        f[4] = f[2]; f[7] = a - k.n_sub; f[8] = b + k.n_add;
    }
}

// The port rule of ONE fluid cell of column 0 (west) and / or column nx - 1 (east), after the pull and the wall rule: Zou and He's
// closure on the reference's expressions (:181-206, :212-235) with ONE of (rho, u) given and the other solved for.
//   west  S = f0 + f2 + f4 + 2 (f3 + f6 + f7)   VELOCITY: u = inlet_u(), rho = S / (1 - u)     PRESSURE: rho = pk.west, u = 1 - S / rho
//   east  S = f0 + f2 + f4 + 2 (f1 + f5 + f8)   PRESSURE: rho = pk.east, u = -1 + S / rho      VELOCITY: u = pk.east,  rho = S / (1 + u)
// and the three unknown populations from (rho, u) as the reference writes them. Every operation is one IEEE operation in the element
// type in the order written (the library is built without contraction), so strict and contracted arithmetic apply the same bits. The
// reference's pair is (VELOCITY, PRESSURE 1): S / 1 and (2/3) * 1 * u change no bit, so the default is no special case.
// The kinds (bits of `walls`, port_pack) and the two values are launch-uniform; the branch on the kind sits inside the one-column branch.
// `inlet_u` gives the west velocity of the cell's row at the iteration served and is called for a west VELOCITY port only: u_row[yg],
// times the schedule's factor where there is one, ONE multiplication rounded before its uses. A schedule scales nothing else.
// rho_bc / u_bc: (rho, u) of the rule applied, the east one where both ran (nx == 1), for the snapshot; untouched off the ports.
// __host__ too: lbm_debug_port_rule applies this very function on the CPU.
template <typename T, typename U>
__host__ __device__ __forceinline__ void port_rule(T (&f)[Q], bool west, bool east, int walls, const PortK<T>& pk, U&& inlet_u,
                                                   T& rho_bc, T& u_bc) {
    if (west) {
        const T S = f[0] + f[2] + f[4] + T(2.0) * (f[3] + f[6] + f[7]);
        // (one division for both kinds: by the density given, or by 1 - u)
        const bool pressure = walls & PORT_WEST_PRESSURE;
        T rho = pk.west, u = T(0.0), den = pk.west;
        if (!pressure) { u = inlet_u(); den = T(1.0) - u; }
        const T q = S / den;
        if (pressure) u = T(1.0) - q; else rho = q;
        f[1] = f[3] + T(2.0 / 3.0) * rho * u;
        f[5] = f[7] - T(0.5) * (f[2] - f[4]) + T(1.0 / 6.0) * rho * u;
        f[8] = f[6] + T(0.5) * (f[2] - f[4]) + T(1.0 / 6.0) * rho * u;
        rho_bc = rho; u_bc = u;
    }
    if (east) {
        const T S = f[0] + f[2] + f[4] + T(2.0) * (f[1] + f[5] + f[8]);
        // (one division for both kinds: by the density given, or by 1 + u, which port_ks has formed: pk.east_den)
        const bool velocity = walls & PORT_EAST_VELOCITY;
        const T q = S / pk.east_den;
        const T rho = velocity ? q : pk.east, u = velocity ? pk.east : T(-1.0) + q;
        f[3] = f[1] - T(2.0 / 3.0) * rho * u;
        f[6] = f[8] - T(0.5) * (f[2] - f[4]) - T(1.0 / 6.0) * rho * u;
        f[7] = f[5] + T(0.5) * (f[2] - f[4]) - T(1.0 / 6.0) * rho * u;
        rho_bc = rho; u_bc = u;
    }
}

// apply_boundary_conditions on the pulled populations of ONE cell, in the reference's sequential loop order
// bottom -> top -> inlet -> outlet (LBMSolver.h:152-236). Solid cells are skipped by every one
// of those loops. Returns nothing; rho_bc/u_bc are exposed for the macro snapshot kernel.
// The inlet velocity of global row yg is u_row[yg] (KArgs::u_row): loaded inside the inlet branch only, so no cell off column 0
// carries its address or value. The two walls are wall_rule above, the two open ends port_rule: the one statement of each, for the
// step kernels and the snapshot.
template <typename T, typename U>
__device__ __forceinline__ void apply_bcs(T (&f)[Q], bool bottom, bool top, bool inlet, bool outlet, U&& inlet_u,
                                          int walls, const WallK<T>& wk, const PortK<T>& pk, T& rho_bc, T& u_bc) {
    wall_rule(f, bottom, top, walls, wk);
    port_rule(f, inlet, outlet, walls, pk, inlet_u, rho_bc, u_bc);
}
// apply_bcs at global cell (x, yg) for the step kernels, at level `lvl` (0-based) of the launch: iteration *t_base + t + lvl, the number
// the first-unstable bookkeeping forms. The device word is read under the schedule's test only — a captured graph carries a fixed `t` and
// advances the word itself, so replays take the right entry with no host involvement. Everything the schedule touches is launch- and
// level-uniform.
// `row_u` gives u_row[yg]: the load itself (bcs_at), or a value that the caller fetched once for all levels of a launch (k_stepc_col,
// whose threads keep their rows: the velocity of a row is wave-uniform there and never changes inside a launch; the schedule's factor does,
// from level to level, and stays here).
template <typename T, typename U>
__device__ __forceinline__ void bcs_at_with(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl, U&& row_u) {
    T rho_bc, u_bc;
    apply_bcs(f, yg == 0, yg == a.ny_glob - 1, x == 0, x == a.nx - 1, [&]() {
        T u = row_u();
        if (a.sched) u = u * inlet_sched_at<T>(a.sched, *a.t_base + a.t + lvl);
        return u;
    }, a.walls, a.wk, a.pk, rho_bc, u_bc);
}
template <typename T>
__device__ __forceinline__ void bcs_at(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl) {
    bcs_at_with(a, f, x, yg, lvl, [&]() { return a.u_row[yg]; });
}

// The collision: the Arith enum, the operators of every model, the map of their launch-uniform values to the slots of KArgs, collide().
}  // namespace lbmk
#include "lbm_collision.hpp"
namespace lbmk {

// Buffer-descriptor access for the block-uniform "lean" paths: address = descriptor base + SGPR offset + ONE 32-bit VGPR
// offset, so the nine populations of a cell cost nine scalar adds and no vector address arithmetic at all (a global_load
// needs a vector add per population: the plane / row displacements are far beyond its immediate-offset range).
typedef unsigned lbm_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_desc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0xffffffff, 0x00020000);   // raw, no range limit
}
// AUX: cache policy of the load (0 default; 2 = nt, non-temporal: the line is not kept for re-use — round 4: the register kernel's
// level-1 loads read every line once per launch, and with nt loads + plain stores it runs 2-4 % faster at 4096x1024 fp64, 164-167
// against 158-163 GLUPS; with nt loads AND nt stores 140: the plan measurement chooses)
template <typename T, int AUX = 0> __device__ __forceinline__ T buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX));
    else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, AUX));
}
template <bool NT> __device__ __forceinline__ void buf_store(double v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(lbm_u32x2, v), r, voff, soff, NT ? 2 : 0);   // aux 2 = nt
}
template <bool NT> __device__ __forceinline__ void buf_store(float v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, NT ? 2 : 0);
}

// Grid::check_stability on one cell's populations: NaN, Inf, > 1e5, < -1e5 (LBMGrid.h:296-307); 1e5 is exact in fp32 too,
// so the test is done in T. Filter first: bit 30 of an IEEE word (the top exponent bit) is set iff |f| >= 2 or f is
// Inf/NaN, so the OR of the nine (high) words has it clear iff every |f_i| < 2 — four v_or3_b32 and a test instead of nine
// compares; the exact test runs only for a wave that holds such a value (never, in a healthy flow). Same verdict, bit for bit.
__device__ __forceinline__ unsigned exp_word(double v) { return (unsigned)(__builtin_bit_cast(unsigned long long, v) >> 32); }
__device__ __forceinline__ unsigned exp_word(float v) { return __builtin_bit_cast(unsigned, v); }
template <typename T>
__device__ __forceinline__ bool any_unstable(const T (&f)[Q]) {
    unsigned o = 0;
#pragma unroll
    for (int i = 0; i < Q; ++i) o |= exp_word(f[i]);
    bool bad = false;
    if (o & 0x40000000u) {
#pragma unroll
        for (int i = 0; i < Q; ++i) bad |= !(fabs(f[i]) <= T(1e5));
    }
    return bad;
}
// the same verdict counted only where `valid`, branch-free in `valid` (k_stepc_col: its garbage cells may hold anything, NaN included)
template <typename T>
__device__ __forceinline__ bool unstable_if(const T (&f)[Q], bool valid) {
    unsigned o = 0;
#pragma unroll
    for (int i = 0; i < Q; ++i) o |= exp_word(f[i]);
    o = valid ? o : 0u;
    bool bad = false;
    if (o & 0x40000000u) {
#pragma unroll
        for (int i = 0; i < Q; ++i) bad |= !(fabs(f[i]) <= T(1e5));
        bad = bad && valid;
    }
    return bad;
}

enum StepMode { MODE_STEP = 0, MODE_COLLIDE_ONLY = 1, MODE_STREAM_ONLY = 2 };

// One iteration per launch: one thread per lattice site, block = 256 sites of one row (4 waves), 8-byte (fp64) /
// 4-byte (fp32) coalesced plane accesses; the x±1 pulls are the same coalesced stream shifted by one element.
//   MODE_STEP         : K_t as described at the top of this file.
//   MODE_COLLIDE_ONLY : collision_step of iteration 0 on the initial state (no pull, no BC, no stability test).
//   MODE_STREAM_ONLY  : f_current snapshot for the accessor: pull + BCs + cylinder reversal
//                       (LBMSolver.h:240-257), every interior cell written, no collision.
template <typename T, int MODE, bool NT = false, int AR = AR_STRICT>
__global__ void __launch_bounds__(256) k_step_site(const KArgs<T> a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = row_of_block(a);
    if (x >= a.nx) return;
    const int yg = a.y_start + y;
    const long c = (long)(y + GR) * a.pitch + a.xoff + x;
    T f[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const long off = (MODE == MODE_COLLIDE_ONLY) ? 0 : (long)cy(i) * a.pitch + cx(i);
        f[i] = a.src[(long)i * a.plane + c - off];
    }
    const bool solid = solid_at(a, x, yg);
    if (MODE != MODE_COLLIDE_ONLY && !solid) bcs_at(a, f, x, yg, 0);
    if (MODE == MODE_STEP) {
        if (any_unstable(f)) atomicMin(a.unstable_t, *a.t_base + a.t);
    }
    if (MODE == MODE_STREAM_ONLY) {
        if (solid) {
            T r[Q];
#pragma unroll
            for (int i = 0; i < Q; ++i) r[i] = f[opp(i)];
#pragma unroll
            for (int i = 0; i < Q; ++i) f[i] = r[i];
        }
    } else {
        if (solid) return;   // collision skips solid cells: they keep w_i for ever (LBMSolver.h:92, N4)
        collide<T, AR>(f, a, column_rate<T, AR>(a, x));
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        T* p = a.dst + (long)i * a.plane + c;
        if (NT) __builtin_nontemporal_store(f[i], p);   // streaming store: do not keep the line in L2
        else *p = f[i];
    }
}

// (Rounds 1-3 also had k_step_vec, the same step with 16 bytes per lane — two fp64 / four fp32 sites per thread: 110 us per iteration
// at 4096x1024 fp64 against 112 for this kernel and 100 for this kernel with non-temporal stores; no measured plan ever took it. Retired
// in round 4 with its 14 instantiations; round 5 removed the option "variant" that used to select it.)

// feq_in: the nine initial-equilibrium values (permanent content of physical N/S ghost rows and corner ghosts), in
// device memory: they are needed by the few cells of a region that lie outside the domain only, and passing them by
// value would pin 18 scalar registers for the whole kernel (the fused kernels are SGPR-bound).
template <typename T> struct K2Extra {
    const T* feq_in;
    int small;   // the buffer is below 4 GiB: the lean paths may address it with 32-bit byte offsets
    int xcd;     // remap the blocks so that every XCD walks one contiguous run of tiles (run-time: scalar index arithmetic only)
    int nt;      // non-temporal stores (run-time in the fused tile kernels: one block-uniform branch around the nine stores)
    int ntl;     // non-temporal LOADS at level 1 of the register kernel (run-time: one block-uniform branch around its 36 loads)
};

// ---------------------------------------------------------------------------------------------------------
// What the fused step kernels (k_step2/3/4_tile, k_stepd_tile, k_stepc_col) share: the update of one cell, its loads and
// stores, and the block prologue (TileFrame). Every per-cell rule of those kernels lives here.
// (The general nine pulls stay written out in the kernels, and outside_value gives one value, not a cell: a loop over a cell
// that is unrolled inside a helper before it is inlined compiles differently — two more VGPRs in k_step2_tile fp32.)

// One general cell of level lvl + 1 (any cell of a non-LEAN path): BCs of that level's iteration unless solid, the stability test where `count`, the
// collision; a solid cell keeps w_i (its collision result is discarded). `near_solid` is block-uniform: tiles far from every
// solid cell skip the select. BRANCH_FREE: the stability test is unstable_if (k_stepc_col, whose garbage cells are masked).
// cell_update_with: the same with the row's inlet velocity from `row_u` (bcs_at_with) and the column's rate `wpx` (column_rate; x may
// lie outside the domain here).
template <typename T, int AR, bool BRANCH_FREE = false, typename U>
__device__ __forceinline__ void cell_update_with(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl, bool solid, bool near_solid,
                                                 bool count, bool& bad, T wpx, U&& row_u) {
    if (!solid) bcs_at_with(a, f, x, yg, lvl, row_u);
    if (BRANCH_FREE) bad |= unstable_if(f, count);
    else if (count) bad |= any_unstable(f);
    collide<T, AR>(f, a, wpx);
    if (near_solid) {
#pragma unroll
        for (int i = 0; i < Q; ++i) f[i] = solid ? wgt<T>(i) : f[i];
    }
}
template <typename T, int AR, bool BRANCH_FREE = false>
__device__ __forceinline__ void cell_update_as(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl, bool solid, bool near_solid,
                                               bool count, bool& bad) {
    cell_update_with<T, AR, BRANCH_FREE>(a, f, x, yg, lvl, solid, near_solid, count, bad, column_rate<T, AR>(a, x), [&]() { return a.u_row[yg]; });
}
// ... with the geometry looked up here (block-uniform branch: only tiles near a solid cell)
template <typename T, int AR>
__device__ __forceinline__ void cell_update(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl, bool near_solid, bool count, bool& bad) {
    bool solid = false;
    if (near_solid) solid = solid_at(a, x, yg);
    cell_update_as<T, AR>(a, f, x, yg, lvl, solid, near_solid, count, bad);
}
// A general cell of the last level, which stores: every cell is counted, and a solid cell is neither collided nor stored
// (false: do not store the cell).
template <typename T, int AR>
__device__ __forceinline__ bool cell_update_last(const KArgs<T>& a, T (&f)[Q], int x, int yg, int lvl, bool near_solid, bool& bad) {
    const bool solid = near_solid && solid_at(a, x, yg);
    if (!solid) bcs_at(a, f, x, yg, lvl);
    bad |= any_unstable(f);
    if (solid) return false;
    collide<T, AR>(f, a, column_rate<T, AR>(a, x));
    return true;
}

// a region cell outside the domain (or beyond what any output needs) takes its permanent ghost value (N1/N2): 0 in the E/W
// ghost columns of interior rows, else the initial equilibrium
template <typename T>
__device__ __forceinline__ T outside_value(const K2Extra<T>& e, bool row_in, bool col_in, int i) {
    return (row_in && !col_in) ? T(0) : e.feq_in[i];
}
// the nine stores of interior cell (x, local row y), plain or non-temporal
template <bool NT, typename T>
__device__ __forceinline__ void store_cell(const KArgs<T>& a, const T (&f)[Q], int x, int y) {
    T* base = a.dst + ((long)(y + GR) * a.pitch + a.xoff + x);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        if (NT) __builtin_nontemporal_store(f[i], base + (long)i * a.plane); else base[(long)i * a.plane] = f[i];
    }
}
template <typename T>
__device__ __forceinline__ void store_cell(const KArgs<T>& a, const T (&f)[Q], int x, int y, bool nt) {   // (block-uniform nt)
    if (nt) store_cell<true>(a, f, x, y); else store_cell<false>(a, f, x, y);
}

// The block-uniform prologue of a fused kernel whose outputs are the OW x OH cells at (X0, Y0) and whose first level reaches HW
// rings beyond them.
template <typename T>
struct TileFrame {
    int X0, Y0;          // first output column / local row
    int y_end;           // rows >= y_end belong to another band / launch
    bool near_solid;     // a cell of the outputs grown by HW rings may be solid
    // LEAN: the outputs and their HW rings lie strictly inside the domain, the output tile is full, nothing is near a solid cell
    // and the buffer is below 4 GiB — every cell of every level is a plain fluid cell: no boundary, ghost, solid or validity logic
    bool lean;
    // (lean path) one uniform base per buffer + a 32-bit byte offset per access: nine scalar offsets + one vector offset per cell
    // (see buf_load). The source descriptor starts KB bytes early: every scalar offset stays >= 0.
    unsigned pitchB, planeB, KB;
    __amdgpu_buffer_rsrc_t rsrc, rdst;

    __device__ __forceinline__ TileFrame(const KArgs<T>& a, const K2Extra<T>& e, int X0_, int Y0_, int y_end_, int OW, int OH, int HW)
        : X0(X0_), Y0(Y0_), y_end(y_end_) {
        near_solid = tile_near_solid(a, X0, Y0, OW, OH, HW);
        const int yg0 = a.y_start + Y0;
        lean = !near_solid && X0 >= HW + 1 && X0 + OW + HW <= a.nx - 1 && yg0 >= HW + 1 && yg0 + OH + HW <= a.ny_glob - 1 &&
               Y0 + OH <= y_end && e.small;
        pitchB = (unsigned)a.pitch * (unsigned)sizeof(T);
        planeB = (unsigned)a.plane * (unsigned)sizeof(T);
        KB = pitchB + (unsigned)sizeof(T);
        rsrc = buf_desc(reinterpret_cast<const char*>(a.src) - KB);
        rdst = buf_desc(a.dst);
    }
    // (lean path) scalar byte offsets of cell (x, local row y) for load / store, and the vector byte offset of (row, col) from it
    __device__ __forceinline__ unsigned src_off(const KArgs<T>& a, int y, int x) const {
        return (unsigned)(y + GR) * pitchB + (unsigned)(a.xoff + x) * (unsigned)sizeof(T) + KB;
    }
    __device__ __forceinline__ unsigned dst_off(const KArgs<T>& a, int y, int x) const {
        return (unsigned)(y + GR) * pitchB + (unsigned)(a.xoff + x) * (unsigned)sizeof(T);
    }
    __device__ __forceinline__ unsigned at(int row, int col) const { return (unsigned)row * pitchB + (unsigned)col * (unsigned)sizeof(T); }
    // (lean path) the nine pulls / stores of one cell
    template <int AUX = 0>
    __device__ __forceinline__ void load(T (&f)[Q], unsigned voff, unsigned soff) const {
#pragma unroll
        for (int i = 0; i < Q; ++i)
            f[i] = buf_load<T, AUX>(rsrc, voff, soff + (unsigned)i * planeB - (unsigned)cy(i) * pitchB - (unsigned)(cx(i) * (int)sizeof(T)));
    }
    template <bool NT>
    __device__ __forceinline__ void store(const T (&f)[Q], unsigned voff, unsigned soff) const {
#pragma unroll
        for (int i = 0; i < Q; ++i) buf_store<NT>(f[i], rdst, voff, soff + (unsigned)i * planeB);
    }
    __device__ __forceinline__ void store(const T (&f)[Q], unsigned voff, unsigned soff, bool nt) const {   // (block-uniform nt)
        if (nt) store<true>(f, voff, soff); else store<false>(f, voff, soff);
    }
};

// The verdict of ONE WAVE of k_stepc_col in a block that is not lean (TileFrame::lean is one verdict for the whole block, and a tile
// whose rings touch a wall row fails it for all its waves, those included whose rows are plain interior fluid at every level). The wave
// holds the R region rows from ry0 of the tile whose outputs are the OW x OH cells at local (Xo, Yo) with HW = D - 1 rings; its band ends
// at y_end. True when every test the general path makes on these rows and on the tile's columns, at every level 1..D, comes out as it
// does for a plain fluid cell, so that the lean path reads, counts and stores for this wave exactly what the general path would:
//   columns  the x-conditions of `lean`: no lane lacks a column, none is the inlet or the outlet column
//   geometry the tile is not near a solid cell (the general path's `sbits` stay 0, its selects change nothing)
//   small    the lean path addresses the buffers with 32-bit byte offsets
//   rows     all R rows lie in [1, ny_glob - 2]: inside the domain (`rin`), off both wall rows. A strip's face and a periodic lattice
//            (a strip PERIODIC_PAD rows up in a taller lattice) reach a wave through these row numbers and through y_end alone
//   load     level 1 loads all R rows (`rld`: y <= y_end + HW - 1)
//   count    levels 2..D count a row inside the level's window (L - 1 <= ry <= H - L) where y <= y_end + HW - L; the lean path counts
//            every row of the window. ry + L over the levels that hold ry is at most min(ry + D, 2 ry + 1, H), which grows with ry, so
//            the wave's last row decides (the rows no level >= 2 holds, ry = 0 and ry = H - 1, are never the binding ones: R >= 2)
//   store    the lean path stores the wave's rows of [Yo, Yo + OH); the general path those below y_end as well: the same rows
// A full band (Yo + OH <= y_end) passes load, count and store for every wave; the partial top band of a whole domain passes them for
// every wave whose rows end below the wall row (y_end = ny_glob there); other partial bands are decided by the same three tests.
// Every term is conservative or exact: false wherever a test of the general path could come out otherwise. The kernel's branch and
// lbm_debug_wave_plain (and through it the tests) call this function. Two restatements exist and must follow it: tools/prof_phases.py
// classifies recorded waves with a copy in Python, and lbm_debug_wave_plain restates TileFrame::lean for the block verdict it reports.
__host__ __device__ inline bool wave_plain(int nx, int ny_glob, int y_start, int Xo, int Yo, int y_end, int OW, int OH, int HW,
                                           bool near_solid, bool small, int ry0, int R) {
    const int D = HW + 1, H = OH + 2 * HW;
    const int ya = Yo - HW + ry0, yb = ya + R - 1, ryb = ry0 + R - 1;            // first / last local row, last region row
    int top = ryb + D;                                                        // max (ry + L) over the levels that hold the last row
    if (2 * ryb + 1 < top) top = 2 * ryb + 1;
    if (H < top) top = H;
    const int last_out = yb < Yo + OH - 1 ? yb : Yo + OH - 1;                 // the last row the lean path stores, if it stores any
    return !near_solid && small && Xo >= HW + 1 && Xo + OW + HW <= nx - 1 &&
           y_start + ya >= 1 && y_start + yb <= ny_glob - 2 &&
           yb <= y_end + HW - 1 &&
           top <= y_end - Yo + 2 * HW &&
           (ya >= Yo + OH || last_out < y_end);
}

// The frame of the LDS tile kernels: tile (bx, by) of TX x TY outputs, grid = tiles x bands. Workgroups are dealt round-robin
// over the 8 XCDs (each with its own L2); with e.xcd the linear block id is remapped so that every XCD walks one contiguous run
// of tiles: horizontally adjacent tiles, which share the cache lines at their common edge, then run on the same L2 at the same time.
template <typename T>
__device__ __forceinline__ TileFrame<T> tile_frame(const KArgs<T>& a, const K2Extra<T>& e, int TX, int TY, int HW) {
    int bx = blockIdx.x, by = blockIdx.y;
    if (e.xcd) {
        const int nb = gridDim.x * gridDim.y;
        int b = by * gridDim.x + bx;
        if (nb % 8 == 0) b = (b % 8) * (nb / 8) + b / 8;
        by = b / gridDim.x; bx = b - by * gridDim.x;
    }
    if (a.reverse) by = (int)gridDim.y - 1 - by;               // (the host never combines reverse with a second range)
    int y_end;
    const int Y0 = band_origin(a, by, TY, y_end);
    return TileFrame<T>(a, e, bx * TX, Y0, y_end, TX, TY, HW);
}

// Two timesteps per launch: temporal blocking through LDS. A block owns a TX x TY tile of outputs at iteration
// t+1. Phase 1 computes P_{t+1} on the (TX+2) x (TY+2) region around it from global P_t — the step kernel's
// per-cell sequence, with cells outside the domain taking their permanent ghost constants (N1/N2) and solid cells
// w_i — into LDS; after one barrier phase 2 pulls from LDS, applies the BCs of iteration t+1, collides and stores
// P_{t+2}. P_{t+1} never touches HBM: traffic per lattice update drops from 144 B to ~(1 + (TX+2)(TY+2)/(TX TY))*36 B
// (82 B at 64x8, less when the tile halo is still in L2 / Infinity Cache). Same arithmetic per cell => results
// bit-identical to two k_step_site launches (tests). Any nx (partial tiles at the right edge); rows of neighbouring strips must be
// present (at least) two deep. LDS: 9*(TY+2)*(TX+4)*sizeof(T) (47.9 KB at TY=8, fp64: three blocks per CU). No LEAN path.
template <typename T, int TY, int NTH, int AR = AR_STRICT>
__global__ void __launch_bounds__(NTH) k_step2_tile(const KArgs<T> a, const K2Extra<T> e) {
    constexpr int TX = 64, RW = TX + 2, RH = TY + 2, LP = RW + 2;
    __shared__ T lds[Q][RH][LP];
    const TileFrame<T> fr = tile_frame(a, e, TX, TY, 1);
    const int X0 = fr.X0, Y0 = fr.Y0, y_end = fr.y_end;
    bool bad = false;
    for (int r = threadIdx.x; r < RW * RH; r += NTH) {         // phase 1: iteration t on the region
        const int ry = r / RW, rx = r - ry * RW;
        const int x = X0 + rx - 1, y = Y0 + ry - 1;
        if (y > y_end) continue;                               // partial last tile: not needed by any output
        const int yg = a.y_start + y;
        const bool row_in = (yg >= 0 && yg < a.ny_glob), col_in = (x >= 0 && x < a.nx);
        T f[Q];
        if (!(row_in && col_in)) {
#pragma unroll
            for (int i = 0; i < Q; ++i) f[i] = outside_value(e, row_in, col_in, i);
        } else {
            const long c = (long)(y + GR) * a.pitch + a.xoff + x;
#pragma unroll
            for (int i = 0; i < Q; ++i) f[i] = a.src[(long)i * a.plane + c - (long)cy(i) * a.pitch - cx(i)];
            cell_update<T, AR>(a, f, x, yg, 0, fr.near_solid, true, bad);
        }
#pragma unroll
        for (int i = 0; i < Q; ++i) lds[i][ry][rx] = f[i];
    }
    if (bad) atomicMin(a.unstable_t, *a.t_base + a.t);
    __syncthreads();
    bad = false;
    for (int o = threadIdx.x; o < TX * TY; o += NTH) {         // phase 2: iteration t+1 on the tile
        const int ly = o / TX, lx = o - ly * TX;
        const int x = X0 + lx, y = Y0 + ly;
        if (y >= y_end || x >= a.nx) continue;               // partial tiles at the right / top edge
        T f[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) f[i] = lds[i][ly + 1 - cy(i)][lx + 1 - cx(i)];
        if (cell_update_last<T, AR>(a, f, x, a.y_start + y, 1, fr.near_solid, bad)) store_cell(a, f, x, y, e.nt != 0);
    }
    if (bad) atomicMin(a.unstable_t, *a.t_base + a.t + 1);
}

// In-kernel phase record (tools/colbench -DLBM_COL_PROF only; never in the library): lane 0 of every wave writes the 100 MHz
// real-time counter at the marks below, plus HW_ID / XCC_ID, so that the host can lay the blocks of one CU side by side (profiles/r04).
#ifdef LBM_COL_PROF
constexpr int PROF_SLOTS = 96;
__device__ unsigned long long* lbm_prof_buf;     // [block][wave][PROF_SLOTS]
__device__ __forceinline__ void prof_mark(int blk, int nw, int w, int slot) {
    asm volatile("" ::: "memory");
    if (((int)threadIdx.x & 63) == 0 && slot < PROF_SLOTS) {
        unsigned long long t;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");    // 100 MHz, chip-wide (s_memtime: per-CU offsets)
        lbm_prof_buf[((size_t)blk * nw + w) * PROF_SLOTS + slot] = t;
    }
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void prof_ids(int blk, int nw, int w) {
    if (((int)threadIdx.x & 63) == 0) {
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11));
        unsigned long long rt;
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt) :: "memory");
        lbm_prof_buf[((size_t)blk * nw + w) * PROF_SLOTS + PROF_SLOTS - 1] = ((unsigned long long)xcc << 32) | hw;
        lbm_prof_buf[((size_t)blk * nw + w) * PROF_SLOTS + PROF_SLOTS - 2] = rt;
    }
}
#define LBM_PROF(blk, nw, w, slot) prof_mark(blk, nw, w, slot)
#define LBM_PROF_IDS(blk, nw, w) prof_ids(blk, nw, w)
#else
#define LBM_PROF(blk, nw, w, slot) do {} while (0)
#define LBM_PROF_IDS(blk, nw, w) do {} while (0)
#endif

// D >= 3 iterations per launch on a TX x TY tile of NTH threads: k_step2_tile's idea D - 2 levels deeper, the LDS image reused in place.
// One body for k_step3_tile, k_step4_tile and k_stepd_tile (below, each with its shapes and what was measured on them):
//   level 1        region 1 = tile + HW = D-1 rings: P_{t+1} from global P_t into an LDS image of (TX+2HW) x (TY+2HW) cells;
//   levels 2..D-1  region L = region 1 shrunk by L-1 rings, in place: every thread first pulls the nine values of its cells
//                  (ceil(cells / NTH) of them) from LDS into registers, barrier, then computes the next state and writes it
//                  IN PLACE (no second LDS image), barrier;
//   level D        the tile: pull from LDS, BCs, collide, store P_{t+D}.
// A region cell outside the domain, or in a row that no output of this launch needs (beyond y_end + HW - L at level L), takes or
// keeps a ghost value and is not counted by the stability test. A block runs the whole tile either LEAN (TileFrame) or general.
// HBM traffic per update ~ (1 + (TX+2HW)(TY+2HW)/(TX TY)) * 72/D B (fp64). Bit-identical to D single launches (tests). Rows of
// neighbouring strips must be present D deep beyond the rows written.
// TILE_FIRST chooses how the cells of a region are dealt to the threads (cell_xy).
template <typename T, int TX, int TY, int NTH, int D, int AR, bool TILE_FIRST>
__device__ __forceinline__ void step_tile(const KArgs<T>& a, const K2Extra<T>& e) {
    constexpr int HW = D - 1, R1W = TX + 2 * HW, R1H = TY + 2 * HW, LP = R1W;
    static_assert(D >= 3, "level 1, at least one in-place level, the last level");
    static_assert(!TILE_FIRST || (TX & (TX - 1)) == 0, "the tile-first cell_xy splits an index with a mask");
    static_assert((size_t)Q * R1H * LP * sizeof(T) <= 160 * 1024, "level-1 region must fit the CU's LDS");
    __shared__ T lds[Q][R1H][LP];
    // Cell r of the region at ring offset O (rows and columns [O, R1 - O) of the LDS image) -> its LDS coordinates.
    auto cell_xy = [&]<int O>(int r, int& ry, int& rx) {
        if constexpr (!TILE_FIRST) {                      // row-major over the region
            constexpr int RW = R1W - 2 * O;
            ry = O + r / RW; rx = O + r - (r / RW) * RW;
        } else {
            // The TX columns above the tile come first, row by row: a half-wave then covers one aligned run of 32 cells (no LDS
            // bank conflict, whole cache lines at level 1) instead of a region row that wraps somewhere inside it; the
            // 2 x (HW - O) halo columns of every row follow.
            constexpr int RH = R1H - 2 * O, HALO = HW - O, NC = RH * TX;
            if (HALO == 0 || r < NC) { ry = O + r / TX; rx = HW + (r & (TX - 1)); }
            else {
                const int h = r - NC, q = h / (2 * HALO), c = h - q * (2 * HALO);
                ry = O + q;
                rx = c < HALO ? O + c : HW + TX + (c - HALO);
            }
        }
    };
    const TileFrame<T> fr = tile_frame(a, e, TX, TY, HW);
    const int X0 = fr.X0, Y0 = fr.Y0, y_end = fr.y_end;
    // The whole tile twice: LEAN (fr.lean) or general; a block takes one of the two (block-uniform), so neither pays for merging
    // with the other.
    auto run = [&]<bool LEAN>() {
        bool bad = false;
        [[maybe_unused]] const int pb = (int)(blockIdx.y * gridDim.x + blockIdx.x), pw = (int)threadIdx.x >> 6;
        LBM_PROF_IDS(pb, NTH / 64, pw);
        LBM_PROF(pb, NTH / 64, pw, 0);
#pragma unroll
        for (int r = threadIdx.x; r < R1W * R1H; r += NTH) {                 // level 1 on region 1: iteration t
            int ry, rx;
            cell_xy.template operator()<0>(r, ry, rx);
            T f[Q];
            if (LEAN) {
                fr.load(f, fr.at(ry, rx), fr.src_off(a, Y0 - HW, X0 - HW));
                bad |= any_unstable(f);
                collide<T, AR>(f, a, column_rate<T, AR>(a, X0 + rx - HW));
            } else {
                const int x = X0 + rx - HW, y = Y0 + ry - HW;
                const int yg = a.y_start + y;
                const bool row_in = (yg >= 0 && yg < a.ny_glob), col_in = (x >= 0 && x < a.nx);
                if (!(row_in && col_in) || y > y_end + HW - 1) {
#pragma unroll
                    for (int i = 0; i < Q; ++i) f[i] = outside_value(e, row_in, col_in, i);
                } else {
                    const long c = (long)(y + GR) * a.pitch + a.xoff + x;
#pragma unroll
                    for (int i = 0; i < Q; ++i) f[i] = a.src[(long)i * a.plane + c - (long)cy(i) * a.pitch - cx(i)];
                    cell_update<T, AR>(a, f, x, yg, 0, fr.near_solid, true, bad);
                }
            }
#pragma unroll
            for (int i = 0; i < Q; ++i) lds[i][ry][rx] = f[i];
        }
        if (bad) atomicMin(a.unstable_t, *a.t_base + a.t);
        LBM_PROF(pb, NTH / 64, pw, 1);
        __syncthreads();
        auto in_place = [&]<int L>() {                                        // level L on region L, in place
            constexpr int O = L - 1, RW = R1W - 2 * O, RH = R1H - 2 * O;
            // cells per thread, at least two: where one would do, the second folds away (its index is past the region for every
            // thread), but with arrays of one element the compiler keeps the test against -1 and divides the cell index in 32 bits
            // (k_step3_tile<float,12,1024,0>: -0.9 % at 4096x1024, profiles/lds_tile_body)
            constexpr int CPT = (RW * RH + NTH - 1) / NTH > 2 ? (RW * RH + NTH - 1) / NTH : 2;
            T g[CPT][Q];
            int cell[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int r = (int)threadIdx.x + k * NTH;
                cell[k] = (r < RW * RH) ? r : -1;
                if (cell[k] >= 0) {
                    int ry, rx;
                    cell_xy.template operator()<O>(r, ry, rx);
#pragma unroll
                    for (int i = 0; i < Q; ++i) g[k][i] = lds[i][ry - cy(i)][rx - cx(i)];
                }
            }
            __syncthreads();
            bool badl = false;
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                if (cell[k] < 0) continue;
                const int r = cell[k];
                int ry, rx;
                cell_xy.template operator()<O>(r, ry, rx);
                // f, the cell being updated: the registers it was pulled into, or (COPY) a copy filled only where the pulled values
                // are used. No one form serves both maps (profiles/lds_tile_body): the copy costs k_stepd_tile<float,32,32,8,0> six
                // SGPR spills and a VGPR, its absence k_step4_tile<double,8,1024,0> nineteen SGPR spills (4 -> 23). The two copies
                // stay written out: behind a lambda the compiler forms the other variant.
                constexpr bool COPY = !TILE_FIRST;
                T copy[Q];
                T (&f)[Q] = COPY ? copy : g[k];
                if (LEAN) {
                    if constexpr (COPY) {
#pragma unroll
                        for (int i = 0; i < Q; ++i) f[i] = g[k][i];
                    }
                    badl |= any_unstable(f);
                    collide<T, AR>(f, a, column_rate<T, AR>(a, X0 + rx - HW));
                } else {
                    const int x = X0 + rx - HW, y = Y0 + ry - HW;
                    const int yg = a.y_start + y;
                    const bool row_in = (yg >= 0 && yg < a.ny_glob), col_in = (x >= 0 && x < a.nx);
                    if (!(row_in && col_in)) {
#pragma unroll
                        for (int i = 0; i < Q; ++i) f[i] = outside_value(e, row_in, col_in, i);
                    } else {
                        if constexpr (COPY) {
#pragma unroll
                            for (int i = 0; i < Q; ++i) f[i] = g[k][i];
                        }
                        cell_update<T, AR>(a, f, x, yg, L - 1, fr.near_solid, y <= y_end + HW - L, badl);
                    }
                }
#pragma unroll
                for (int i = 0; i < Q; ++i) lds[i][ry][rx] = f[i];
            }
            if (badl) atomicMin(a.unstable_t, *a.t_base + a.t + L - 1);
            __syncthreads();
            LBM_PROF(pb, NTH / 64, pw, L);
        };
        [&]<int... Ls>(std::integer_sequence<int, Ls...>) { (in_place.template operator()<Ls + 2>(), ...); }(std::make_integer_sequence<int, D - 2>{});
        bad = false;
        for (int o = threadIdx.x; o < TX * TY; o += NTH) {                    // level D on the tile: iteration t+D-1
            const int ly = o / TX, lx = o - ly * TX;                          // (one cell per thread where NTH == TX * TY)
            const int x = X0 + lx, y = Y0 + ly;
            if (!LEAN && (y >= y_end || x >= a.nx)) continue;                 // partial tiles at the right / top edge
            T f[Q];
#pragma unroll
            for (int i = 0; i < Q; ++i) f[i] = lds[i][ly + HW - cy(i)][lx + HW - cx(i)];
            if (LEAN) {
                bad |= any_unstable(f);
                collide<T, AR>(f, a, column_rate<T, AR>(a, x));
                fr.store(f, fr.at(ly, lx), fr.dst_off(a, Y0, X0), e.nt != 0);
            } else if (cell_update_last<T, AR>(a, f, x, a.y_start + y, D - 1, fr.near_solid, bad)) store_cell(a, f, x, y, e.nt != 0);
        }
        if (bad) atomicMin(a.unstable_t, *a.t_base + a.t + D - 1);
        LBM_PROF(pb, NTH / 64, pw, D);                  // stores issued
#ifdef LBM_COL_PROF
        __builtin_amdgcn_s_waitcnt(0x0f70);             // vmcnt(0): ... and drained
        LBM_PROF(pb, NTH / 64, pw, D + 1);
#endif
    };
    if (fr.lean) run.template operator()<true>();
    else run.template operator()<false>();
}

// Three / four iterations per launch (D = 3 / 4) over 64 x TY tiles, regions dealt row-major. LDS 9*(TY+2HW)*(64+2HW)*sizeof(T):
// 78 KB at 64x12 fp64 for D = 3, two blocks of 1024 threads per CU = all 32 wave slots, the lean path needs 48 VGPRs; 70.5 KB at
// 64x8 fp64, 35 KB fp32 for D = 4. At most two cells per thread in the in-place levels. fp64 traffic 58 B per update at 64x12,
// D = 3; redundant collisions 1.21x (64x12, D = 3) / 1.45x (64x8, D = 4) — D = 4 is worth it where the three-iteration kernel is
// close to the memory roof (fp32). Strips (six rows per exchange = 2 x 3) never use D = 4; the plan measurement decides elsewhere.
template <typename T, int TY, int NTH, int AR = AR_STRICT>
__global__ void __launch_bounds__(NTH, (2 * NTH / 256)) k_step3_tile(const KArgs<T> a, const K2Extra<T> e) { step_tile<T, 64, TY, NTH, 3, AR, false>(a, e); }
template <typename T, int TY, int NTH, int AR = AR_STRICT>
__global__ void __launch_bounds__(NTH, (2 * NTH / 256)) k_step4_tile(const KArgs<T> a, const K2Extra<T> e) { step_tile<T, 64, TY, NTH, 4, AR, false>(a, e); }

// D = 6..8 on 64x16 / 32x32 tiles of 1024 threads, one thread per tile cell, regions dealt tile columns first: for grids so
// small that one launch is a single round of blocks. There the chip runs load -> compute -> store in lockstep, so the two memory
// phases are paid per LAUNCH: fusing more iterations divides them, at the price of ~1.5x redundant collisions that such a grid
// has VALU time to spare for.
// (Round 2's production shape — 32x16 tiles, 512 threads, D = 5/6, two blocks per CU: 125-130 GLUPS at 4096x1024 fp64 — is
// superseded by k_stepc_col, which keeps the same region in registers instead of LDS, and is no longer built.)
// Whole-domain launches only (rows outside the domain hold the permanent ghost values; a strip is refreshed six rows deep per single launch).
// waves per SIMD the register allocation may assume: as many blocks as the LDS image allows on a CU (at most 32 waves)
template <typename T, int TX, int TY, int D>
constexpr int deep_waves_per_simd() {
    const int lds = (int)sizeof(T) * Q * (TX + 2 * (D - 1)) * (TY + 2 * (D - 1)), waves = TX * TY / 64;
    int blocks = 160 * 1024 / lds;
    if (blocks * waves > 32) blocks = 32 / waves;
    return (blocks * waves) / 4 > 0 ? (blocks * waves) / 4 : 1;
}
template <typename T, int TX, int TY, int D, int AR = AR_STRICT>
__global__ void __launch_bounds__(TX * TY, (deep_waves_per_simd<T, TX, TY, D>())) k_stepd_tile(const KArgs<T> a, const K2Extra<T> e) { step_tile<T, TX, TY, TX * TY, D, AR, true>(a, e); }

// ---------------------------------------------------------------------------------------------------------
// Initialisation: Grid::initialise (LBMGrid.h:185-246) written into BOTH buffers, plus the permanent ghost
// values of N1/N2 (see top of file). feq_in = f_eq(1,(u_in,0)) evaluated on the host in double with the
// reference's bracket order (LBMUtils.h:9-12,46); solid cells get f_eq(1,0,0) = w_i. With a per-row inlet profile the interior
// fluid cells of row yg take f_eq(1,(u[yg],0)) instead, from a table built on the host the same way (the ghost frame keeps feq_in).
template <typename T>
struct InitArgs {
    T* a; T* b;
    long plane; int pitch, xoff, nx, ny_loc, ny_glob, y_start;
    int cyl_x, cyl_y; double cyl_r2;
    MaskView mv;
    T feq_in[Q];
    const T* feq_row = nullptr;   // lbm_set_inlet_profile: row yg (global) at feq_row[yg * Q + i], rows of the strip's window; nullptr: feq_in
    int* solid_count;
};

template <typename T>
__global__ void __launch_bounds__(256) k_init(const InitArgs<T> p) {
    const int gx = blockIdx.x * 256 + threadIdx.x;   // 0 .. nx+1  (ghost-inclusive column)
    const int gy = blockIdx.y;                       // 0 .. ny_loc+2*GR-1
    if (gx > p.nx + 1) return;
    const int x = gx - 1, yg = p.y_start + gy - GR;  // global coordinates (may lie outside the domain)
    const bool row_interior = (yg >= 0 && yg < p.ny_glob);
    const bool col_interior = (x >= 0 && x < p.nx);
    const bool own_row = (gy >= GR && gy < p.ny_loc + GR);
    bool solid = false;
    if (row_interior && col_interior) solid = solid_at(p, x, yg);
    if (solid && own_row) atomicAdd(p.solid_count, 1);
    const long c = (long)gy * p.pitch + p.xoff + x;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        T v = p.feq_in[i];
        if (p.feq_row && row_interior && col_interior) v = p.feq_row[(long)yg * Q + i];
        if (solid) v = wgt<T>(i);
        if (row_interior && !col_interior) v = T(0);   // N1: E/W ghost column of a globally-interior row
        p.a[(long)i * p.plane + c] = v;
        p.b[(long)i * p.plane + c] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Macroscopic snapshot from the buffer `old` = P_t that the last step kernel READ:
//   fluid interior : moments of P_t at the cell. collision conserves rho and rho*u, so these equal the
//                    pre-collision moments the reference stored at LBMSolver.h:112-114 to round-off (~1e-16).
//   inlet/outlet   : (rho, u, 0) of the port's rule (port_rule) of iteration t — (rho_bc, u_in, 0) / (1, u_out, 0) with the
//                    reference's ports — recomputed exactly as the step kernel did (pull from P_t + wall BC + Zou-He); the
//                    initial snapshot has the row's value (u_row) and rho = 1 there.
//   solid          : (1, 0, 0) (rho never rewritten after init, u zeroed at LBMSolver.h:260-261).
template <typename T>
struct MacroArgs {
    const T* old; long plane; int pitch, xoff, nx, ny_loc, ny_glob, y_start;
    int cyl_x, cyl_y; double cyl_r2;
    const T* u_row;     // inlet velocity per global row, as KArgs::u_row
    MaskView mv;
    int initial;        // steps_done == 0: analytic initial macros (LBMGrid.h:219-228)
    double* rho; double* ux; double* uy;   // [ny_loc][nx]
    unsigned long long* max_usq_bits;      // optional running max of ux^2+uy^2 (bit pattern of a double >= 0)
    int walls; WallK<T> wk;                // the two walls, as KArgs carries them (appended: the fields above keep their offsets)
    T in_scale;                            // the inlet schedule's factor of the iteration this snapshot describes, (T)s(t), formed by the host
                                           // (lbm_set_inlet_schedule); 1 without a schedule: x * 1 changes no bit, so no branch
    T frc_hx, frc_hy;                      // a context with a driving force (lbm_set_forcing): h = F/2, as KArgs carries it, which the fluid cells'
    int forced;                            // velocity takes off the momentum of the populations read (macro_moments) where `forced` is set
    PortK<T> pk;                           // the values of the two ports, as KArgs carries them (their kinds ride in `walls`), in what was padding
    char frc_pad[64 - 6 * sizeof(T)];      // (64 bytes in all with `forced` and its alignment: what follows this struct in FrameArgs, ProbeArgs, StatsArgs keeps its place)
};

// the moments of the nine populations of a fluid cell, in the element type: rho and u = (sum c_i f_i) / rho (one definition for
// k_macros, k_stats, k_frame and k_probes: they must agree to the bit).
// Under a driving force (lbm_set_forcing) the velocity is Guo's, u = (sum c f_pre + F/2) / rho of the collision that wrote the
// populations read here. Those are POST-collision ones, whose momentum is the pre-collision one plus F, so h = F/2 is taken off: one
// IEEE subtraction per component before the division. A launch-uniform branch, taken with a force set only: without one no bit changes.
template <typename T>
__device__ __forceinline__ void macro_moments(const MacroArgs<T>& p, const T (&f)[Q], double& r, double& vx, double& vy) {
    T rr = T(0), sx = T(0), sy = T(0);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const T v = f[i];
        rr += v;
        if (cx(i) != 0) sx += T(cx(i)) * v;
        if (cy(i) != 0) sy += T(cy(i)) * v;
    }
    if (p.forced) { sx = sx - p.frc_hx; sy = sy - p.frc_hy; }
    sx /= rr; sy /= rr;
    r = (double)rr; vx = (double)sx; vy = (double)sy;
}

// (rho, ux, uy) of cell (x, local row y) as the snapshot defines them above. The one definition of the snapshot: k_macros writes it
// out, k_stats adds it to the running sums.
template <typename T>
__device__ __forceinline__ void macro_cell(const MacroArgs<T>& p, int x, int y, double& r, double& vx, double& vy) {
    const int yg = p.y_start + y;
    const long c = (long)(y + GR) * p.pitch + p.xoff + x;
    const bool solid = solid_at(p, x, yg);
    if (solid) { r = 1.0; vx = 0.0; vy = 0.0; }
    else if (p.initial) { r = 1.0; vx = (double)p.u_row[yg]; vy = 0.0; }
    else if (x == 0 || x == p.nx - 1) {
        T f[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) f[i] = p.old[(long)i * p.plane + c - (long)cy(i) * p.pitch - cx(i)];
        T rho_bc = T(1), u_bc = T(0);
        apply_bcs(f, yg == 0, yg == p.ny_glob - 1, x == 0, x == p.nx - 1, [&]() { return p.u_row[yg] * p.in_scale; }, p.walls, p.wk, p.pk, rho_bc, u_bc);
        // (rho, u) of the port's rule: the given one as cast, the other as solved; the east rule runs after the west one (only matters for nx == 1)
        r = (double)rho_bc; vx = (double)u_bc; vy = 0.0;
    } else {
        T f[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) f[i] = p.old[(long)i * p.plane + c];
        macro_moments<T>(p, f, r, vx, vy);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_macros(const MacroArgs<T> p) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    double usq = 0.0;
    if (x < p.nx) {
        double r, vx, vy;
        macro_cell<T>(p, x, y, r, vx, vy);
        const long m = (long)y * p.nx + x;
        p.rho[m] = r; p.ux[m] = vx; p.uy[m] = vy;
        usq = vx * vx + vy * vy;
    }
    if (p.max_usq_bits) {
        // wave max, then one atomic per wave; non-negative doubles order like their bit patterns
        for (int o = 32; o > 0; o >>= 1) usq = fmax(usq, __shfl_xor(usq, o));
        if ((threadIdx.x & 63) == 0) atomicMax(p.max_usq_bits, (unsigned long long)__double_as_longlong(usq));
    }
}

// ---------------------------------------------------------------------------------------------------------
// Time-averaged statistics (lbm_stats_begin; the reference has none): one SAMPLE adds the snapshot macro_cell defines — taken from
// P_t, the buffer the sampling point finds in buf[cur] — to six running sums per cell, always in double:
//   acc[0..5][ny_loc][nx] = sum rho | sum ux | sum uy | sum ux*ux | sum uy*uy | sum ux*uy      (the layout of d_macro, six planes)
// Every sum is S = S + v in sample order, every product rounded to double before it is added (no contraction in this kernel), so the
// sums equal a host loop `S += ux*ux` over the snapshots bit for bit; means and Reynolds stresses are formed by the caller.
// A pure streaming kernel: 9 sizeof(T) bytes of populations read and 96 bytes of accumulators read and written per cell. A thread
// owns two adjacent cells of a row — one 16-byte access per lane and accumulator plane, 16 (fp64) / 8 (fp32) bytes per lane and
// population plane — and a block of 256 threads (four waves) 512 cells. The pull + wall + Zou-He path of the inlet and outlet columns
// is taken by the two lanes of a row that own them (and by a lattice whose width is odd, where the pairs are not 16-byte aligned);
// every other lane runs the vector path. The accumulators are stored with plain stores: non-temporal 16-byte stores were measured
// and are 1-2 % slower at both 4096x1024 fp64 and 16384x4096 fp32 (profiles/stats/README.md).
template <typename T>
struct StatsArgs {
    MacroArgs<T> m;     // the snapshot's source: old = P_t, initial = 0; rho / ux / uy / max_usq_bits unused
    double* acc;        // [6][ny_loc][nx]
    long cells;         // nx * ny_loc: the plane stride of acc
};

template <typename T> struct Pair2;
template <> struct Pair2<double> { typedef double2 type; };
template <> struct Pair2<float> { typedef float2 type; };

template <typename T>
__global__ void __launch_bounds__(256) k_stats(const StatsArgs<T> p) {
#pragma clang fp contract(off)
    const MacroArgs<T>& a = p.m;
    const int x0 = 2 * (blockIdx.x * 256 + threadIdx.x);
    const int y = blockIdx.y;
    if (x0 >= a.nx) return;
    double r[2], vx[2], vy[2];
    const bool vec = (a.nx & 1) == 0;       // (uniform) pairs start at even cells of an even-width row: 16-byte aligned
    if (!vec || x0 == 0 || x0 + 2 >= a.nx) {
        macro_cell<T>(a, x0, y, r[0], vx[0], vy[0]);
        if (x0 + 1 < a.nx) macro_cell<T>(a, x0 + 1, y, r[1], vx[1], vy[1]);
        else { r[1] = 0.0; vx[1] = 0.0; vy[1] = 0.0; }
    } else {
        typedef typename Pair2<T>::type T2;
        const long c = (long)(y + GR) * a.pitch + a.xoff + x0;
        T f0[Q], f1[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            const T2 v = *reinterpret_cast<const T2*>(a.old + (long)i * a.plane + c);
            f0[i] = v.x; f1[i] = v.y;
        }
        macro_moments<T>(a, f0, r[0], vx[0], vy[0]);
        macro_moments<T>(a, f1, r[1], vx[1], vy[1]);
        const int yg = a.y_start + y;
        if (solid_at(a, x0, yg)) { r[0] = 1.0; vx[0] = 0.0; vy[0] = 0.0; }
        if (solid_at(a, x0 + 1, yg)) { r[1] = 1.0; vx[1] = 0.0; vy[1] = 0.0; }
    }
    const long m = (long)y * a.nx + x0;
    double v0[6] = {r[0], vx[0], vy[0], vx[0] * vx[0], vy[0] * vy[0], vx[0] * vy[0]};
    double v1[6] = {r[1], vx[1], vy[1], vx[1] * vx[1], vy[1] * vy[1], vx[1] * vy[1]};
    if (vec) {
        double2 s[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = *reinterpret_cast<const double2*>(p.acc + (long)k * p.cells + m);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s[k].x = s[k].x + v0[k]; s[k].y = s[k].y + v1[k];
            *reinterpret_cast<double2*>(p.acc + (long)k * p.cells + m) = s[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double* q = p.acc + (long)k * p.cells + m;
            q[0] = q[0] + v0[k];
            if (x0 + 1 < a.nx) q[1] = q[1] + v1[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// IOManager::record_forces, LBMIO.h:133-160: momentum exchange over solid->fluid links, evaluated on the
// post-collision populations P_t. One block scans the obstacle's bounding box (+1 cell) restricted to the rows
// this strip owns, visiting FLUID cells and their solid neighbours (geometry from global coordinates), so strip
// partial sums add up to the one-rank value. Deterministic tree reduction in LDS.
// A box of more than FORCE_CHUNK cells (a mask that covers much of the domain, e.g. a porous bed) is cut into fixed chunks of
// FORCE_CHUNK cells, one block each, whose partial sums k_forces_sum adds in chunk order: a partition and a summation order that
// depend on the box alone, so every plan and every repetition gives the same bits. One chunk is exactly the one-block scan.
template <typename T>
struct ForceArgs {
    const T* cur; long plane; int pitch, xoff, nx, ny_loc, ny_glob, y_start;
    int cyl_x, cyl_y, cyl_r; double cyl_r2;
    MaskView mv;
    int x0, x1, y0, y1;     // inclusive box in (x, local y)
    double* out;            // out[0] = t (as double), out[1] = fx, out[2] = fy
    double* part;           // several chunks: [gridDim.x][2] partial sums (k_forces_sum writes `out`)
    int t;
};
constexpr long FORCE_CHUNK = 65536;

template <typename T>
__global__ void __launch_bounds__(1024) k_forces(const ForceArgs<T> p) {
    __shared__ double sfx[1024];
    __shared__ double sfy[1024];
    double fx = 0.0, fy = 0.0;
    const int bw = p.x1 - p.x0 + 1, bh = p.y1 - p.y0 + 1;
    const long ncell = (bw > 0 && bh > 0) ? (long)bw * bh : 0;
    const long k0 = gridDim.x > 1 ? (long)blockIdx.x * FORCE_CHUNK : 0;
    const long k1 = gridDim.x > 1 ? (k0 + FORCE_CHUNK < ncell ? k0 + FORCE_CHUNK : ncell) : ncell;
    for (long k = k0 + threadIdx.x; k < k1; k += 1024) {
        const int x = p.x0 + (int)(k % bw), y = p.y0 + (int)(k / bw);
        const int yg = p.y_start + y;
        if (solid_at(p, x, yg)) continue;
        const long c = (long)(y + GR) * p.pitch + p.xoff + x;
#pragma unroll
        for (int i = 1; i < Q; ++i) {
            const int sx = x + cx(i), sy = yg + cy(i);
            if (sx < 0 || sx >= p.nx || sy < 0 || sy >= p.ny_glob) continue;
            if (!solid_at(p, sx, sy)) continue;
            const double fi = (double)p.cur[(long)i * p.plane + c];
            fx += 2.0 * cx(i) * fi;
            fy += 2.0 * cy(i) * fi;
        }
    }
    sfx[threadIdx.x] = fx; sfy[threadIdx.x] = fy;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sfx[threadIdx.x] += sfx[threadIdx.x + s]; sfy[threadIdx.x] += sfy[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (gridDim.x > 1) { p.part[2 * blockIdx.x] = sfx[0]; p.part[2 * blockIdx.x + 1] = sfy[0]; }
        else { p.out[0] = (double)p.t; p.out[1] = sfx[0]; p.out[2] = sfy[0]; }
    }
}
// the chunks' partial sums of k_forces in chunk order (one thread: at most a few hundred chunks)
template <typename T>   // (T: one instantiation per element type of the launcher, like every kernel of this header)
__global__ void __launch_bounds__(64) k_forces_sum(const double* part, int nchunks, double* out, int t) {
    if (threadIdx.x != 0) return;
    double fx = 0.0, fy = 0.0;
    for (int b = 0; b < nchunks; ++b) { fx += part[2 * b]; fy += part[2 * b + 1]; }
    out[0] = (double)t; out[1] = fx; out[2] = fy;
}

// ---------------------------------------------------------------------------------------------------------
// The same momentum exchange PER BODY (lbm_set_body_labels; the reference has one disc and one total): the force on body k is the
// part of the sum above whose links END in a cell of label k — fluid cell x (label 0) of this strip's rows, direction i, neighbour
// x + c_i inside the domain with label k — so bodies that touch are told apart by the solid end of every link.
// Geometry comes from ONE byte per cell, lab[(ny_loc + 2)][nx]: the strip's rows and one ghost row per face (the neighbour strip's
// labels; zeros beyond the domain, which is what keeps the row test of k_forces out of this kernel). Only this kernel reads it.
// The host cuts every body's bounding box (+1 cell, clipped to the domain and to the strip's rows) into chunks of FORCE_CHUNK cells
// (lbm_geom.hpp pack_bodies) and uploads ONE table of them, sorted by body and by first cell: one block per chunk with the stride
// loop and the LDS tree of k_forces unchanged, the chunks' partial sums kept in `part` and added per body in chunk order by
// k_forces_bodies_sum. Partition and order depend on the labels and the strip alone: every plan, layout and repetition gives the
// same bits, and with 1 as the only label the chunks, the addends of every thread and their order are those of k_forces — the row
// of body 1 IS the total, bit for bit. A body without a cell in the box of this strip has no chunk and gets zeros.
struct BodyChunk { int body; int cells; long first; };     // label, cells of this chunk, its first cell in the box's row-major order
template <typename T>
struct BodyForceArgs {
    const T* cur; long plane; int pitch, xoff, nx;
    const unsigned char* lab;     // [(ny_loc + 2)][nx]: row r holds local row r - 1
    const int* box;               // [B][4]: x0, x1, y0, y1 of body b + 1, inclusive, in (x, local y)
    const BodyChunk* chunks;
    double* part;                 // [chunks][2]
};

template <typename T>
__global__ void __launch_bounds__(1024) k_forces_bodies(const BodyForceArgs<T> p) {
    __shared__ double sfx[1024];
    __shared__ double sfy[1024];
    double fx = 0.0, fy = 0.0;
    const BodyChunk ch = p.chunks[blockIdx.x];
    const int b = ch.body;
    const int x0 = p.box[4 * (b - 1)], bw = p.box[4 * (b - 1) + 1] - x0 + 1, y0 = p.box[4 * (b - 1) + 2];
    const long k1 = ch.first + ch.cells;
    for (long k = ch.first + threadIdx.x; k < k1; k += 1024) {
        const int x = x0 + (int)(k % bw), y = y0 + (int)(k / bw);
        const unsigned char* row = p.lab + (long)(y + 1) * p.nx;
        if (row[x] != 0) continue;
        const long c = (long)(y + GR) * p.pitch + p.xoff + x;
#pragma unroll
        for (int i = 1; i < Q; ++i) {
            const int sx = x + cx(i);
            if (sx < 0 || sx >= p.nx) continue;
            if (row[(long)cy(i) * p.nx + sx] != b) continue;
            const double fi = (double)p.cur[(long)i * p.plane + c];
            fx += 2.0 * cx(i) * fi;
            fy += 2.0 * cy(i) * fi;
        }
    }
    sfx[threadIdx.x] = fx; sfy[threadIdx.x] = fy;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sfx[threadIdx.x] += sfx[threadIdx.x + s]; sfy[threadIdx.x] += sfy[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { p.part[2 * blockIdx.x] = sfx[0]; p.part[2 * blockIdx.x + 1] = sfy[0]; }
}
// one thread per body: the partial sums of its chunks [first[b], first[b + 1]) in chunk order; out = [B][3] rows (t, fx, fy)
template <typename T>
__global__ void __launch_bounds__(64) k_forces_bodies_sum(const double* part, const int* first, int nbodies, double* out, int t) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nbodies) return;
    const int c0 = first[b], c1 = first[b + 1];
    double fx = 0.0, fy = 0.0;
    if (c1 - c0 == 1) { fx = part[2 * c0]; fy = part[2 * c0 + 1]; }      // (k_forces writes the sum of a single chunk as it is)
    else for (int c = c0; c < c1; ++c) { fx += part[2 * c]; fy += part[2 * c + 1]; }
    out[3 * b] = (double)t; out[3 * b + 1] = fx; out[3 * b + 2] = fy;
}

// ---------------------------------------------------------------------------------------------------------
// Host-staged halo rows (lbm_halo_export / lbm_halo_import): GR rows x 9 planes x nx interior columns per face,
// as double, [GR][9][nx]. `row0` = first local gy of the GR consecutive rows.
template <typename T>
__global__ void __launch_bounds__(256) k_halo_pack(const T* buf, long plane, int pitch, int xoff, int nx, int row0,
                                                   double* out) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;          // 0 .. GR*Q-1  = row-major (row, plane)
    if (x >= nx) return;
    const int r = k / Q, i = k - r * Q;
    out[(long)k * nx + x] = (double)buf[(long)i * plane + (long)(row0 + r) * pitch + xoff + x];
}
template <typename T>
__global__ void __launch_bounds__(256) k_halo_unpack(T* buf, long plane, int pitch, int xoff, int nx, int row0,
                                                     const double* in) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (x >= nx) return;
    const int r = k / Q, i = k - r * Q;
    buf[(long)i * plane + (long)(row0 + r) * pitch + xoff + x] = (T)in[(long)k * nx + x];
}

}  // namespace lbmk
