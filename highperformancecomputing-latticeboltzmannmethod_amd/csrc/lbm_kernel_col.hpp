// csrc/lbm_kernel_col.hpp — D iterations per launch with the lattice held in REGISTERS (round 3's production kernel).
//
// The LDS-image kernels (k_stepd_tile) move every population of every cell through LDS at every level: nine ds_write and
// nine ds_read per cell and level, with a thread <-> cell map that changes from level to level, two barriers per level,
// and an LDS image that caps the tile at ~1000 cells per block. On gfx950 that LDS traffic costs about as much as the
// collision arithmetic and the two never overlap inside a block (profiles/r02). This kernel keeps the map FIXED instead:
//
//   block  = NW waves; it owns a region of 64 columns x H = R*NW rows of the lattice for all D levels
//   wave w = rows [w*R, (w+1)*R) of the region, lane = column: every thread holds R vertically adjacent cells, i.e.
//            R x 9 populations, in VGPRs from the first load to the last store
//   level 1  pulls P_t from HBM for all cells of the region (nine displaced coalesced row loads per row)
//   level l  needs, per cell, the level l-1 populations of its eight neighbours:
//              same thread, row above/below  -> a register (free)
//              x -/+ 1                        -> DPP wave shift of the neighbour lane's register (v_mov_b32_dpp wave_shr/shl:1)
//              row above/below the thread's R -> the neighbouring WAVE: three populations per face through LDS
//            so per wave and level 6 ds_write + 6 ds_read in all (1.5 + 1.5 per cell at R = 4, against 9 + 9) and ONE
//            barrier (the exchange buffer is double-buffered); the rest population never leaves its register.
//   level D  stores the (64 - 2(D-1)) x (H - 2(D-1)) cells in the middle of the region: P_{t+D}
// Cells at distance < l-1 from the region's edge hold garbage at level l (their neighbours were never loaded); nothing
// valid ever reads them — the garbage moves inward one ring per level, exactly as the valid region shrinks — and the
// stability verdict is masked to the valid cells of each level. Same per-cell operation sequence as every other step
// kernel => bit-identical results (tests).
// Redundant collisions: x 64/56, y (H + .. + H-8)/(5 (H-8)) at D = 5: 1.33x at H = 32. HBM traffic per update at D = 5,
// H = 32: (2048 + 1344) * 72 B / (1344 * 5) = 36 B before L2 absorbs the overlap, like the 32x16 LDS tile.
//
// Parked top row (PARK: fp64 with R = 5, a 64x40 region on eight waves). Five fp64 rows are 90 state registers, one row more than 128
// VGPRs hold beside a collision (unparked: 128 VGPRs, 19 spilled). Rows 0..R-2 stay in registers; row R-1 lives in LDS between levels:
//   pbuf[w][0..5]        populations 0, 1, 3, 4, 7, 8 of wave w's top row (pad columns as in xbuf; one buffer; only wave w touches it)
//   xbuf[.][w][0..2]     its north-going 2, 5, 6, which only the wave above needs: the owner's pull takes 2, 5, 6 from row R-2
//   level 1              loads all rows, updates the top row first and parks it: pbuf, and xbuf[0], which level 2 reads
//   level L, before the barrier   writes only the bottom row's 4, 7, 8 into xbuf[L&1]
//   level L, row R-2     takes 4, 7, 8 from pbuf at lane 0, +1, -1 (no DPP)
//   level L, row R-1     takes 0, 1, 3 from pbuf at lane 0, -1, +1; 2, 5, 6 from row R-2 and 4, 7, 8 from the wave above, as every form does;
//                        its new values go to pbuf and xbuf[(L+1)&1] (L < D) or to the lattice (L = D)
// Order inside pbuf: the LDS operations of one wave execute in program order, the reads of a level stand in front of its writes (the
// writes depend on them through the collision), and the barrier of level L+1 stands between the writes of level L and the next reads.
// Reuse of xbuf: xbuf[(L+1)&1] was last read during level L-1 (three reads behind barrier L-1, three in front of that level's last
// row); a wave that writes it during level L has passed barrier L, so every wave has finished level L-1. One barrier per level stays.
// Skipped top rows. A row outside the level's window is not updated and so writes nothing: xbuf[(L+1)&1][w][0..2] then holds what level
// L-2 or level 1 left there. The only reader is row ry+1 of the wave above at level L+1. If row ry was updated at level L-1 but not at L
// (ry = L-2 or ry = H-L+1), its values of level L-1 stand in xbuf[L&1], written then, and level L reads exactly those. If it was not
// updated at level L-1 either (ry < L-2 or ry > H-L+1), the reader is outside its own window (ry+1 < L-1 or ry+1 > H-L): garbage reads
// garbage, as in the unparked form, where the stale registers are rewritten into xbuf at every level.
// Ghost rows (general path): a top row outside the domain takes its ghost values at level 1, is skipped at levels 2..D and is read at
// every one of them, from both parities of xbuf: level 1 writes its three into both. pbuf keeps its other six untouched.
// A lane that reads a pad column of pbuf (lane 0 at x-1, lane 63 at x+1) is outside every window from level 2 on, as for xbuf.
// Mixed blocks. The path is chosen per WAVE: a block that is not lean (a wall tile, a partial band, a strip's edge) still sends down the
// lean path every wave for which wave_plain (lbm_kernels.hpp) holds — all its rows plain interior fluid at every level, loaded at level 1,
// counted and stored as the general path would. In a top wall tile of seven iterations on 64x40 that is four of eight waves, in a bottom
// one six; the general path is 2.85 times the lean path's instructions per level. Why the two paths may share a block:
//   barriers  both run exactly one __syncthreads per level 2..D and none elsewhere (the early return is for the whole block), and the
//             hardware barrier counts the waves of the workgroup that arrive, at whichever instruction each of them does
//   xbuf      both write slots [L&1][w][3..5] (and [0..2], unparked) in front of barrier L and read [L&1][w-1][0..2] / [w+1][3..5] behind
//             it, under the same window test (the general path's additional `rin` is true for a plain wave's rows), so a wave cannot tell
//             which path its neighbour took; the reuse argument above speaks of levels and barriers only and holds as it stands
//   pbuf      a wave touches its own slot only
//   ghost rows (parked form) a general wave's level 1 parks its top row's north-going three into BOTH parities, a lean wave into parity 0
//             only. The second write is for a top row that no later level updates because it lies outside the domain; a plain wave has no
//             such row, and its top row is covered by "Skipped top rows". The general wave's extra write into xbuf[1][w][0..2] is read by
//             wave w+1 at level 3 at the earliest and overwritten before by w's own level 2 where that level updates the row: as in a
//             block that is general throughout
//   u_sh      written and read by general waves of tile column 0 only; no wave of that column is plain
//   counting  level 1 counts every lane of every row on the lean path and `col_in` lanes of loaded rows on the general path; levels 2..D
//             count `lane_ok` against `lane_ok && col_in && y <= y_end + HW - L`; the stores add `col_in && y < y_end && !solid`:
//             wave_plain is true only where each pair agrees for all the wave's rows
// A lean tile's waves never evaluate a different instruction stream than before: the verdict is one more scalar test in front of it.
#pragma once
#include "lbm_kernels.hpp"

namespace lbmk {

// lane i <- lane i-1 (lane 0 reads 0) / lane i <- lane i+1 (lane 63 reads 0): full-wave DPP shifts. bound_ctrl:0 with every
// row and bank enabled leaves no lane that keeps an "old" value, so the instruction has no tied input and the compiler
// needs no copy in front of it (with old = src it emitted one v_mov per shifted dword: 38 of ~390 vector instructions a level).
__device__ __forceinline__ unsigned dpp_shr1(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x138, 0xf, 0xf, true); }
__device__ __forceinline__ unsigned dpp_shl1(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x130, 0xf, 0xf, true); }
__device__ __forceinline__ double from_left(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = dpp_shr1((unsigned)u), hi = dpp_shr1((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double from_right(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = dpp_shl1((unsigned)u), hi = dpp_shl1((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float from_left(float v) { return __builtin_bit_cast(float, dpp_shr1(__builtin_bit_cast(unsigned, v))); }
__device__ __forceinline__ float from_right(float v) { return __builtin_bit_cast(float, dpp_shl1(__builtin_bit_cast(unsigned, v))); }

// (in-kernel phase record, tools/colbench -DLBM_COL_PROF only: LBM_PROF / LBM_PROF_IDS, lbm_kernels.hpp)
// waves per SIMD the register allocation may assume: two blocks per CU when they fit 32 waves (8 waves: four per SIMD, 128 VGPRs;
// 12 waves: six per SIMD, 80 VGPRs — the two-row fp64 strict shape), else one
template <int NW> constexpr int col_waves_per_simd() { return NW == 12 ? 6 : NW <= 8 ? (2 * NW) / 4 : NW / 4; }
// ... per instantiation: the fp32 contracted TRT kernels of eight waves run THREE blocks per CU (six waves per SIMD, 80 VGPRs; 74 when they
// were written). With the bound of four the allocator takes what it likes below 128, and the seven-iteration one came out at 82 once
// KArgs carried the walls: two blocks per CU, 237 -> 208 GLUPS at 4096x1024 (profiles/walls/README.md). Said here, it stays at six.
// The fp32 contracted MRT kernels likewise: 76-80 VGPRs before the per-wave verdict; with it and the bound of four the five-iteration
// ones took 82 (five waves per SIMD instead of six). Under the bound of six: 78 / 76 / 78 at five / six / seven iterations, no scratch
// (profiles/boundary_waves/kernel_resources.txt).
template <typename T, int NW, int AR> constexpr int col_min_waves() {
    return (sizeof(T) == 4 && NW == 8 && (AR == AR_CONTRACTED_TRT || AR == AR_CONTRACTED_MRT)) ? 6 : col_waves_per_simd<NW>();
}

// Tile walk: blocks are dealt round-robin over the 8 XCDs (each with its own 4 MiB L2) in index order; here every XCD walks
// one contiguous run of the row-major tile order instead, so that x-neighbours — which share the lines at their common
// edge — meet in the same L2 at the same time and every XCD streams whole lattice rows (149.6 -> 161.7 GLUPS at 4096x1024
// fp64). A band-major walk (8..37 tile columns per band, so that y-neighbours meet in L2 too) was measured and is gone:
// 141-147 GLUPS — a tile then touches 300 sub-rows that its XCD's other tiles do not share, and the TLB / DRAM-page
// locality of the row-interleaved layout is lost; walking 2..4 tile rows together column by column (y-neighbours adjacent in
// the order) gains nothing at 4096x1024 and loses 12-25 % at 8192x2048 (profiles/r03/README.md).
// The grid is one-dimensional: cdiv(nx, OW) * (bands of both row ranges) blocks, rounded up to a multiple of 8 — one block per
// tile. PERSISTENT blocks (two per CU walking the tiles of their XCD's run in a loop, so that a wave which has stored its last
// rows issues its next tile's loads at once) were built and measured: 123 GLUPS against 142 for the same binary launched
// one block per tile — blocks that start together and take equally long stay phase-locked, and the two blocks of a CU then
// load together and compute together instead of filling each other's gaps, which the dispatcher's staggered hand-out gives
// for free; the loop also costs registers (every loop-invariant scalar offset wants an SGPR for the whole kernel: 106 SGPRs,
// > 100 spilled, 164 -> 142 GLUPS even when launched one block per tile). Gone.
// Round 5 measured two more forms of this kernel and dropped both (profiles/r05/README.md §2-3; the code is archived as a patch in
// profiles/r05/archive/): the waves of a block meeting through NEIGHBOUR FLAGS in LDS instead of one barrier per level (bit-exact; a
// wave's first wait shrinks, but a CU's slot frees only with a block's last wave: residency 1.63 -> 1.47 blocks per CU, -5 %), and the
// x-shifts through the LDS CROSSBAR (ds_bpermute_b32) instead of DPP moves (bit-exact; -1..3 %: the crossbar's latency sits in every
// row's dependency chain and vector issue is not the binding resource at the margin).
template <typename T, int R, int NW, int D, bool NT, int AR = AR_STRICT>
__global__ void __launch_bounds__(NW * 64, (col_min_waves<T, NW, AR>())) k_stepc_col(const KArgs<T> a, const K2Extra<T> e) {
    constexpr int H = R * NW, HW = D - 1, OW = 64 - 2 * HW, OH = H - 2 * HW, LW = 64 + 2;
    static_assert(D >= 2 && OH >= 1 && R >= 2, "(D <= GR on a strip: its ghost rows go GR deep — the host's business)");
    // exchange buffer: per wave the three north-going populations of its top row and the three south-going ones of its
    // bottom row; the first / last wave, which have no neighbour below / above, read their OWN slot instead (garbage for cells
    // that are garbage anyway: round 4 dropped the two phantom slots, 63 -> 51 KB at 8 fp64 waves, so that 12 waves fit two
    // blocks per CU); one pad column on each side for the diagonal reads at lane -/+ 1
    __shared__ T xbuf[2][NW][6][LW];
    // the parked form (header: "Parked top row"): per wave, populations 0, 1, 3, 4, 7, 8 of its top row; pad columns as in xbuf
    constexpr bool PARK = sizeof(T) == 8 && R == 5;
    // the rows of a level in front of which the parked row's reads are issued: row R-2's three and row R-1's three. Two rows ahead where the
    // registers allow it (BGK 120 VGPRs, TRT 124); the Smagorinsky collision holds more live values, and with all six reads in front of row
    // R-3 its kernels take 128 VGPRs and spill four: row R-1's three wait one row longer there (126 VGPRs, no scratch)
    constexpr bool PARK_LATE = AR == AR_STRICT_LES || AR == AR_CONTRACTED_LES;
    constexpr int PARK_AT = R >= 3 ? R - 3 : 0, PARK_AT1 = R >= 3 ? (PARK_LATE ? R - 2 : R - 3) : 0;
    __shared__ T pbuf[PARK ? NW : 1][6][LW];
    __shared__ T u_sh[NW][R];                              // (general tiles with column 0) the inlet velocity of every wave's rows
    const int lane = (int)threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int nbx = (a.nx + OW - 1) / OW, nby = (a.y_cnt + OH - 1) / OH + (a.y_cnt2 + OH - 1) / OH, nb = nbx * nby;
    int b = blockIdx.x;
    { const int per = (int)gridDim.x >> 3; b = (b & 7) * per + (b >> 3); }                   // gridDim.x is a multiple of 8
    if (b >= nb) return;                                                                      // (whole block: no barrier is left waiting)
    int by = b / nbx;
    const int bx = b - by * nbx;
    if (a.reverse) by = nby - 1 - by;
    int y_end;
    const int Yo = band_origin(a, by, OH, y_end);          // first output row / column of this block
    const int Xo = bx * OW;
    const int X0 = Xo - HW, Yr = Yo - HW;                  // region origin
    const int ry0 = w * R;                                 // this wave's first region row
    const TileFrame<T> fr(a, e, Xo, Yo, y_end, OW, OH, HW);   // (its X0 / Y0 are the output origin Xo / Yo)
    const int x = X0 + lane;
    auto run = [&]<bool LEAN>() {
        T g[R][Q];
        bool bad = false;
        // (parked form) the top row's new values of level L: six parked, the north-going three into the exchange buffer that level L + 1
        // reads (last read during level L - 1, and this wave has passed barrier L: every wave has finished level L - 1)
        auto park = [&](const T (&f)[Q], int par) {
            pbuf[w][0][1 + lane] = f[0]; pbuf[w][1][1 + lane] = f[1]; pbuf[w][2][1 + lane] = f[3];
            pbuf[w][3][1 + lane] = f[4]; pbuf[w][4][1 + lane] = f[7]; pbuf[w][5][1 + lane] = f[8];
            xbuf[par][w][0][1 + lane] = f[2]; xbuf[par][w][1][1 + lane] = f[5]; xbuf[par][w][2][1 + lane] = f[6];
        };
        // level 1 of the parked form takes the top row first and parks it: the other rows' collisions then run over R - 1 rows of state
        auto first_top = [](int jj) { return PARK ? (jj == 0 ? R - 1 : jj - 1) : jj; };
        const bool col_in = (x >= 0 && x < a.nx);
        // (sponge kernels) the rate of the thread's column, the same at every level: one load per launch, on both paths. A lane without a
        // column takes the nearest column's (column_rate clamps the index into the table); nothing it computes is counted or stored
        const T wpx = column_rate<T, AR>(a, x);
        // bit j: the thread's cell of row j is solid. The thread <-> cell map is fixed for all D levels, so the geometry is looked
        // up once, here, and serves every level and the store predicate (block-uniform branch: only tiles near a solid cell)
        unsigned sbits = 0;
        // The general path fetches once what no level of a launch changes, and every read of level 1 goes out before the first value is
        // looked at (one exposed round trip per wave, like the lean path's; the per-row and per-level reads it had cost one each):
        //   mw    the mask words of the thread's R cells (a masked context near a solid cell; the disc is arithmetic), looked at once the
        //         lattice loads are out
        //   u_sh  the inlet velocity of the wave's R rows (tiles with column 0): lane j fetches row j's, the wave keeps them in its own
        //         slot of shared memory (no other wave reads it: no barrier) and the inlet branch of every level reads them there. Held
        //         in scalar registers they cost the TRT and LES kernels their occupancy step (profiles/boundary_tiles/README.md)
        //   the ghost constants e.feq_in are read at level 1 only: a cell outside the domain takes its permanent value there and keeps
        //   it, levels 2..D skip it
        // Every address is one that the per-level reads took before, under the same test.
        // The tests on a row are wave-uniform and the same at every level; they are made once and kept as two words of R bits (bit j:
        // row j): rin, the row lies inside the domain; rld, level 1 loads it (inside, and not beyond what the band's outputs need).
        // Written out at every use, each comparison stayed live from level 1 to level D as a 64-bit lane mask of its own (scalar spills).
        unsigned long long mw[R];
        unsigned rin = 0, rld = 0;
        const bool masked = !LEAN && fr.near_solid && a.mv.bits != nullptr;                     // (block-uniform)
        if (!LEAN) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int y = Yr + ry0 + j, yg = a.y_start + y;
                mw[j] = 0;
                if (yg >= 0 && yg < a.ny_glob) { rin |= 1u << j; if (y <= y_end + HW - 1) rld |= 1u << j; }
            }
            if (fr.near_solid && col_in) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const int yg = a.y_start + Yr + ry0 + j;
                    if ((rin >> j) & 1u) {
                        if (masked) mw[j] = mask_word(a.mv, x, yg);
                        else if (is_solid_cell(x, yg, a.cyl_x, a.cyl_y, a.cyl_r2)) sbits |= 1u << j;
                    }
                }
            }
            if (bx == 0 && lane < R && !(a.walls & PORT_WEST_PRESSURE)) {       // (a west pressure port reads no inlet velocity: port_rule)
                const int yg = a.y_start + Yr + ry0 + lane;
                u_sh[w][lane] = (yg >= 0 && yg < a.ny_glob) ? a.u_row[yg] : T(0);
            }
            __builtin_amdgcn_wave_barrier();                       // (other lanes of this wave read the slot: no instruction, an order)
        }
        LBM_PROF_IDS(b, NW, w);
        LBM_PROF(b, NW, w, 0);
        // ---- level 1: iteration t on the whole region, from HBM
        if (LEAN) {
            const unsigned ub = fr.src_off(a, Yr + ry0, X0), voff = (unsigned)lane * (unsigned)sizeof(T);   // wave-uniform, lane
            auto load_all = [&]<int AUX>() {
#pragma unroll
                for (int jj = 0; jj < R; ++jj) { const int j = first_top(jj); fr.template load<AUX>(g[j], voff, ub + (unsigned)j * fr.pitchB); }
            };
            if (e.ntl) load_all.template operator()<2>(); else load_all.template operator()<0>();      // (block-uniform)
#pragma unroll
            for (int jj = 0; jj < R; ++jj) {
                const int j = first_top(jj);
                bad |= any_unstable(g[j]);
                collide<T, AR>(g[j], a, wpx);
                if constexpr (PARK) if (jj == 0) park(g[j], 0);
            }
        } else {
            // rows outside the domain, or beyond what the band's outputs need (wave-uniform): outside_value. The nine constants come by
            // VECTOR loads straight into the row's registers, like the lattice loads below and waited for with them: the address is
            // uniform, and left to itself the compiler fetches them into 9 / 18 scalar registers, which this kernel does not have
            // (scalar spills in the TRT kernels)
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const bool row_in = (rin >> j) & 1u;
                if (!((rld >> j) & 1u)) {
                    const T* fq = e.feq_in;
                    asm volatile("" : "+v"(fq));                                     // (a vector register: the loads below are vector loads)
#pragma unroll
                    for (int i = 0; i < Q; ++i) g[j][i] = T(0);
                    if (!(row_in && !col_in)) {
#pragma unroll
                        for (int i = 0; i < Q; ++i) g[j][i] = fq[i];
                    }
                }
            }
            // the loads of all other rows, each under the test it always had (a lane without a column: outside_value's zero) ...
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int y = Yr + ry0 + j;
                if ((rld >> j) & 1u) {
#pragma unroll
                    for (int i = 0; i < Q; ++i) g[j][i] = T(0);
                    if (col_in) {
                        const long c = (long)(y + GR) * a.pitch + a.xoff + x;
#pragma unroll
                        for (int i = 0; i < Q; ++i) g[j][i] = a.src[(long)i * a.plane + c - (long)cy(i) * a.pitch - cx(i)];
                    }
                }
            }
            if (masked) {
#pragma unroll
                for (int j = 0; j < R; ++j) sbits |= (unsigned)((mw[j] >> (x & 63)) & 1ull) << j;
            }
            // ... then the updates. A lane without a column computes on zeros, is not counted and takes its zeros back: a select, no
            // branch (a block-uniform flag around it, for the tiles that have such lanes, cost scalar spills in the fp64 TRT kernels)
#pragma unroll
            for (int jj = 0; jj < R; ++jj) {
                const int j = first_top(jj);
                const int yg = a.y_start + Yr + ry0 + j;
                if ((rld >> j) & 1u) {
                    cell_update_with<T, AR, true>(a, g[j], x, yg, 0, (sbits >> j) & 1u, fr.near_solid, col_in, bad, wpx, [&]() { return u_sh[w][j]; });
#pragma unroll
                    for (int i = 0; i < Q; ++i) g[j][i] = col_in ? g[j][i] : T(0);
                }
                // (parked form) loaded or ghost, the row is parked; a ghost row is never written again, so its north-going three go into
                // both exchange buffers
                if constexpr (PARK) if (jj == 0) { park(g[j], 0); park(g[j], 1); }
            }
        }
        if (bad) atomicMin(a.unstable_t, *a.t_base + a.t);
        LBM_PROF(b, NW, w, 1);
        // ---- levels 2..D: exchange with the neighbouring waves / lanes, then update in place (level D: store)
        auto level = [&]<int L>() {
            T (*xb)[6][LW] = xbuf[L & 1];
            const int wb = w > 0 ? w - 1 : 0, wa = w + 1 < NW ? w + 1 : NW - 1;
            if constexpr (!PARK) { xb[w][0][1 + lane] = g[R - 1][2]; xb[w][1][1 + lane] = g[R - 1][5]; xb[w][2][1 + lane] = g[R - 1][6]; }
            xb[w][3][1 + lane] = g[0][4];     xb[w][4][1 + lane] = g[0][7];     xb[w][5][1 + lane] = g[0][8];
            __syncthreads();
            // from the wave below (its top row): f2 at x, f5 at x-1, f6 at x+1; from the wave above (its bottom row): f4, f7 at x+1, f8 at x-1
            T p2 = xb[wb][0][1 + lane], p5 = xb[wb][1][lane], p6 = xb[wb][2][2 + lane];
            bool badl = false;
            const bool lane_ok = lane >= L - 1 && lane <= 64 - L;
            T q[6];                                                     // (parked form) the parked row as its two readers pull it
#pragma unroll
            for (int j = 0; j < R; ++j) {
                const int ry = ry0 + j;
                if constexpr (PARK) {
                    if (j == PARK_AT) { q[3] = pbuf[w][3][1 + lane]; q[4] = pbuf[w][4][2 + lane]; q[5] = pbuf[w][5][lane]; }     // row R-2: f4, f7 from x+1, f8 from x-1
                    if (j == PARK_AT1) { q[0] = pbuf[w][0][1 + lane]; q[1] = pbuf[w][1][lane]; q[2] = pbuf[w][2][2 + lane]; }    // row R-1: f0, f1 from x-1, f3 from x+1
                }
                const T n2 = g[j][2], n5 = g[j][5], n6 = g[j][6];       // this row's north-going values, for row j+1
                const int y = Yr + ry, yg = a.y_start + y;
                // (wave-uniform) rows outside the level's window hold garbage from here on; a row outside the domain keeps the ghost
                // values that level 1 gave it
                if (ry >= L - 1 && ry <= H - L && (LEAN || ((rin >> j) & 1u))) {
                T f[Q];
                if (PARK && j == R - 1) { f[0] = q[0]; f[1] = q[1]; f[3] = q[2]; }
                else { f[0] = g[j][0]; f[1] = from_left(g[j][1]); f[3] = from_right(g[j][3]); }
                f[2] = p2; f[5] = p5; f[6] = p6;
                if (PARK && j == R - 2) { f[4] = q[3]; f[7] = q[4]; f[8] = q[5]; }
                else if (j < R - 1) { f[4] = g[j + 1][4]; f[7] = from_right(g[j + 1][7]); f[8] = from_left(g[j + 1][8]); }
                else { f[4] = xb[wa][3][1 + lane]; f[7] = xb[wa][4][2 + lane]; f[8] = xb[wa][5][lane]; }   // (read here, not after the barrier: six registers fewer are live across the rows below; the buffer is not rewritten before this wave has passed the next barrier)
                const bool valid = lane_ok;
                bool store = L == D && lane >= HW && lane < 64 - HW && ry >= HW && ry < H - HW;
                if (LEAN) {
                    badl |= unstable_if(f, valid);
                    collide<T, AR>(f, a, wpx);
                } else {
                    // (a lane without a column: as at level 1 — not counted, not stored, its zeros back)
                    cell_update_with<T, AR, true>(a, f, x, yg, L - 1, (sbits >> j) & 1u, fr.near_solid,
                                                  valid && col_in && y <= y_end + HW - L, badl, wpx, [&]() { return u_sh[w][j]; });
#pragma unroll
                    for (int i = 0; i < Q; ++i) f[i] = col_in ? f[i] : T(0);
                    store = store && col_in && y < y_end && !((sbits >> j) & 1u);
                }
                if (L < D) {
                    if (PARK && j == R - 1) park(f, (L + 1) & 1);
                    else {
#pragma unroll
                    for (int i = 0; i < Q; ++i) g[j][i] = f[i];
                    }
                } else if (store) {
                    if (LEAN) fr.template store<NT>(f, (unsigned)lane * (unsigned)sizeof(T), fr.dst_off(a, y, X0));
                    else store_cell<NT>(a, f, x, y);
                }
                }
                if (j < R - 1) { p2 = n2; p5 = from_left(n5); p6 = from_right(n6); }   // row j+1 pulls them from this row
            }
            if (badl) atomicMin(a.unstable_t, *a.t_base + a.t + L - 1);
            LBM_PROF(b, NW, w, L);
        };
        [&]<int... Ls>(std::integer_sequence<int, Ls...>) { (level.template operator()<Ls + 2>(), ...); }(std::make_integer_sequence<int, D - 1>{});
    };
    // (wave-uniform: header, "Mixed blocks")
    if (fr.lean || wave_plain(a.nx, a.ny_glob, a.y_start, Xo, Yo, y_end, OW, OH, HW, fr.near_solid, e.small != 0, ry0, R)) run.template operator()<true>();
    else run.template operator()<false>();
}

}  // namespace lbmk
