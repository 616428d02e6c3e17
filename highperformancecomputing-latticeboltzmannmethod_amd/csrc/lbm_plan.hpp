// csrc/lbm_plan.hpp — which formulations of the step a context may run: the candidate list of the plan measurement
// (choose_plan, lbm_hip.hip), the strip rule, and the names / option strings of a plan. Pure host C++ (no HIP, no device): the
// library exports it through lbm_debug_plan_candidates so that the bench's bookkeeping can be checked on the CPU
// (tests/test_bench_cpu.py: every fused candidate of every BASELINE.json grid has a committed counter pass).
#pragma once
#include <cstdio>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

#include "lbm_kernels.hpp"

namespace lbmk {

// layout 0 planar / 1 row-interleaved; nt: non-temporal stores;
// alternate: walk direction alternates per launch; fuse: iterations per launch of the tile kernels (1..4) or of the deep shape;
// ty: tile height of the two- / three-iteration tile kernels (8 or 12); xcd: XCD-aware tile walk; deep: 0, or the id of a row of
// deep_shapes (below); ntl: the register kernel's level-1 loads are non-temporal
struct Plan { int layout, nt, alternate, fuse, ty, xcd; std::string name; int deep = 0; int ntl = 0; };

// The collision models, one row each: everything the host knows about a model beyond its C-ABI setter. `base` is the model's strict
// Arith value (lbm_kernels.hpp; base | 1: its contracted one) and what lbm_ctx::collision holds; `noun` names it in messages;
// `tall`, `park`: the 64x48 fp32 and the 64x40 fp64 regions (region_kinds, below) are instantiated for it; `ckpt_bit`: the LBMCKPT3 flag that announces its parameter (0: none —
// rows in ascending order of this bit, the order the parameters stand in the file); the last three are the words checkpoints and
// setters use for the parameter, its value and a context without it.
// the models whose contracted kernels on the tall fp64 regions keep four waves per SIMD without scratch: BGK 120 VGPRs, TRT 124,
// Smagorinsky 126 with three of the parked row's reads issued a row later (profiles/col_parked/README.md; build.py COLLISION_MODELS)
constexpr bool PARK_LES = true, PARK_TRT = true;
// BGK under a driving force (lbm_set_forcing): its contracted kernels on the tall fp64 regions take 122-123 VGPRs, no scratch, four waves
// per SIMD like BGK's 120 (profiles/forcing/README.md). Like LES and TRT it has no tall fp32 regions: their
// two objects are BGK's alone (lbm_col.hip -DLBM_COL_TALL), so no forced instantiation of them exists to meet the bar.
constexpr bool PARK_FORCED = true;
// The MRT collision (lbm_set_mrt): its contracted kernels take all 128 VGPRs on the 64x32 regions of fp64 (no scratch, BGK's four waves
// per SIMD); on the tall fp64 regions they spilled 7 to 9 VGPRs into 24 bytes of scratch per lane when they were built, so the row
// withholds them (profiles/mrt/README.md). No tall fp32 regions, like every model but BGK.
constexpr bool PARK_MRT = false;
// The outlet sponge (lbm_set_sponge): BGK with the rate of the cell's column. Its row starts as MRT's did, with neither kind of tall
// region: the fp64 64x40 instantiations have not been built and read for scratch, so the row withholds them (profiles/sponge/README.md).
constexpr bool PARK_SPONGE = false;
// `nparam`: the doubles of the model's parameter (the force has two components; lbm_ctx::collision_param, collision_param2). A model whose
// ckpt_bit lies above the bits of the walls and the inlet schedule stands behind them in a checkpoint, as its bit says
// (lbm_ckpt.hpp makes one row of its field table from each model that has a bit).
// `unit`: the base of the model in whose objects the model's kernels are instantiated (build.py builds one set of objects per unit;
// lbm_step_k.hip and lbm_col.hip instantiate a unit's riders beside it); -1: its own. MRT shares TRT's pair code and rides in TRT's objects,
// the outlet sponge is BGK's code with another rate and rides in BGK's.
struct CollisionModel { int base; const char* noun; bool tall, park; unsigned long long ckpt_bit; const char *param, *value, *none; int nparam = 1; int unit = -1; };
// (the sponge's row, member by member: the width is carried as a double in front of tau_end)
constexpr CollisionModel sponge_model() {
    CollisionModel m{};
    m.base = AR_STRICT_SPONGE; m.noun = "outlet sponge";
    m.tall = false; m.park = PARK_SPONGE;
    m.ckpt_bit = 2048;
    m.param = "sponge"; m.value = "(width, tau_end) = "; m.none = "";
    m.nparam = 2; m.unit = AR_STRICT;
    return m;
}
constexpr CollisionModel collision_models[] = {
    {AR_STRICT, "BGK", true, true, 0, "", "", ""},
    {AR_STRICT_LES, "Smagorinsky (LES)", false, PARK_LES, 4, "Smagorinsky constant", "Cs = ", " (BGK)"},
    {AR_STRICT_TRT, "two-relaxation-time (TRT)", false, PARK_TRT, 8, "TRT magic parameter", "", ""},
    {AR_STRICT_FORCED, "forced BGK (Guo forcing)", false, PARK_FORCED, 64, "forcing", "F = ", "", 2},
    {.base = AR_STRICT_MRT, .noun = "multiple-relaxation-time (MRT)", .tall = false, .park = PARK_MRT, .ckpt_bit = 1024, .param = "MRT parameters",
     .value = "(bulk rate, magic) = ", .none = "", .nparam = 2, .unit = AR_STRICT_TRT},
    sponge_model(),
};
// the row of an Arith value, strict or contracted
constexpr const CollisionModel& collision_model(int arith) {
    for (const CollisionModel& m : collision_models)
        if (m.base == (arith & ~1)) return m;
    return collision_models[0];
}
// a model's parameter as messages print it: one number, or the pair of a model with two (nparam)
inline std::string param_text(const CollisionModel& m, double v, double v2, const char* fmt = "%g") {
    char a[40], b[40];
    snprintf(a, sizeof(a), fmt, v); snprintf(b, sizeof(b), fmt, v2);
    return m.nparam == 2 ? std::string("(") + a + ", " + b + ")" : std::string(a);
}

// ---- the deep launch shapes: one table of region kinds, one of ids. Launchers, plan_launch, names, messages and refusals read them ----
// A region of the register kernel (k_stepc_col) is 64 columns x rows per thread * waves; {0, 0}: that precision and arithmetic is not built.
struct RowsWaves { int rows, waves; };
// a launch depth a kind offers; nt: a non-temporal-store instantiation exists beside the plain one (they cost 14 % on the fp32 64x48
// regions, and seven iterations are the depth of remainders and of plans that all store plainly); no_face: not on a context with a
// physical strip face (its ghost rows go six deep, seven where a plan of that depth exchanges seven)
struct ColDepth { int depth; bool nt, no_face; };
struct RegionKind {
    const char* name;
    RowsWaves rw[2][2];                 // [fp64, fp32][strict, contracted]
    ColDepth depths[3];
    bool CollisionModel::*needs;        // the flag of the model's row that grants the kind (nullptr: every model has it)
    const char* only;                   // what else a context must be, as messages say it (checked by lbm_initialise); nullptr: nothing
};
enum { RK_STD, RK_TALL, RK_PARK };
constexpr RegionKind region_kinds[] = {
    // 8 waves x 4 rows, two blocks per CU — except fp64 STRICT arithmetic, whose collision needs a dozen more live registers than 128
    // VGPRs leave beside 4 x 9 fp64 populations: 12 waves x 2 rows = 64x24, 70 VGPRs = six waves per SIMD, 135.7 against 127.3 GLUPS on
    // 8 x 3 (tools/colbench --strict); contracted arithmetic is fastest on 8 x 4 (64x24 on 24 waves: 157-159 against 158-162)
    {"64x32", {{{2, 12}, {4, 8}}, {{4, 8}, {4, 8}}}, {{5, true, false}, {6, true, false}, {7, false, true}}, nullptr, nullptr},
    // fp32 (round 4): contracted 76 VGPRs = two blocks of twelve waves, strict 112-116 VGPRs. At seven iterations it stores 52x36 of
    // its cells where 64x32 stores 54x22 at six: 1.33 x instead of 1.45 x the lattice read per launch; 16384x4096: 320 GLUPS against 289-298
    {"64x48", {{{0, 0}, {0, 0}}, {{6, 8}, {4, 12}}}, {{6, false, false}, {7, false, false}, {8, false, true}}, &CollisionModel::tall, nullptr},
    // fp64 contracted: the top row of every thread parked in LDS between levels (lbm_kernel_col.hpp "Parked top row": 120-124 VGPRs, no
    // scratch, 76 352 B of LDS per block = two blocks per CU); strict arithmetic keeps 12 waves x 2 rows
    {"64x40", {{{0, 0}, {5, 8}}, {{0, 0}, {0, 0}}}, {{5, true, false}, {6, true, false}, {7, false, false}}, &CollisionModel::park, "contracted arithmetic on whole domains"},
};
// Option "deep" = the id of a row. LDS rows (k_stepd_tile) launch their own depth on their tile only; register rows launch their depth
// while it fits a segment and any depth their kind offers for what the segment leaves over (20 = 7 + 7 + 6). Ids 4 / 5 were round 2's
// 32x16 LDS tiles: retired. The strip rule and the strip tuner name the ids they pick.
enum { DEEP_LDS6 = 1, DEEP_LDS7 = 2, DEEP_LDS8 = 3, DEEP_COL5 = 6, DEEP_COL6 = 7, DEEP_TALL7 = 8, DEEP_COL7 = 9, DEEP_PARK6 = 10, DEEP_PARK7 = 11 };
struct DeepShape { int id, depth, kind, tile_w, tile_h; };      // kind: a row of region_kinds, or -1: an LDS tile of tile_w x tile_h
constexpr DeepShape deep_shapes[] = {
    {DEEP_LDS6, 6, -1, 64, 16}, {DEEP_LDS7, 7, -1, 64, 16}, {DEEP_LDS8, 8, -1, 32, 32},
    {DEEP_COL5, 5, RK_STD, 0, 0}, {DEEP_COL6, 6, RK_STD, 0, 0}, {DEEP_COL7, 7, RK_STD, 0, 0},
    {DEEP_TALL7, 7, RK_TALL, 0, 0}, {DEEP_PARK6, 6, RK_PARK, 0, 0}, {DEEP_PARK7, 7, RK_PARK, 0, 0},
};
constexpr const DeepShape* deep_shape(int id) {
    for (const DeepShape& s : deep_shapes) if (s.id == id) return &s;
    return nullptr;
}
constexpr int deep_depth(int id) { return deep_shape(id) ? deep_shape(id)->depth : 0; }
constexpr const RegionKind* deep_kind(int id) { return deep_shape(id) && deep_shape(id)->kind >= 0 ? &region_kinds[deep_shape(id)->kind] : nullptr; }
constexpr bool deep_is_col(int id) { return deep_kind(id) != nullptr; }
constexpr RowsWaves col_rw(const RegionKind& k, int esize, bool contracted) { return k.rw[esize == 4][contracted]; }
constexpr const ColDepth* col_depth(const RegionKind& k, int depth) {
    for (const ColDepth& d : k.depths) if (d.depth == depth) return &d;
    return nullptr;
}
// output tile of a register launch of `depth` iterations
constexpr int col_tile_w(int depth) { return 64 - 2 * (depth - 1); }
constexpr int col_tile_h(int depth, RowsWaves rw) { return rw.rows * rw.waves - 2 * (depth - 1); }
// f(std::integral_constant<size_t, I>) for the first I < N that pred(I) accepts; false: none does. How a table row becomes template
// arguments (the launchers of lbm_col.hip and lbm_step_k.hip), in the style of with_collision_base (lbm_launch.inc.hpp).
template <size_t N, typename P, typename F>
bool with_row(P&& pred, F&& f) {
    return [&]<size_t... I>(std::index_sequence<I...>) { return ((pred(I) && (f(std::integral_constant<size_t, I>{}), true)) || ...); }(std::make_index_sequence<N>{});
}
// Why a context of this element size and collision model may not run deep shape `id` ("": it may). The arithmetic mode and the extent
// count once they are `settled` only: options may follow `deep`, so lbm_set_option and the models' setters ask before, lbm_initialise after.
inline std::string deep_refusal(int id, int esize, const CollisionModel& m, bool settled, bool contracted, bool whole_domain) {
    if (id && !deep_shape(id)) return "deep must be 0..3 or 6..11 (4 / 5, round 2's 32x16 LDS tiles, are retired)";
    const RegionKind* k = deep_kind(id);
    if (!k) return "";
    const std::string what = "deep " + std::to_string(id) + " (" + k->name + " regions in registers)";     // (as plan names call them)
    if (!k->rw[esize == 4][0].rows && !k->rw[esize == 4][1].rows) return what + " exists in " + (esize == 4 ? "fp64" : "fp32") + " only";
    if (k->needs && !(m.*k->needs)) return what + " has no " + m.noun + " kernel";
    if (settled && k->only && !(col_rw(*k, esize, contracted).rows && whole_domain)) return what + " exists for " + k->only + " only";
    return "";
}

struct PlanQuery {
    int nx = 0, nyl = 0, ny_glob = 0;   // columns, rows of this strip, rows of the lattice
    int esize = 8;                      // bytes per element
    int num_cus = 256;
    int nstrips = 1;                    // strips of the run (ranks or group members)
    bool strips = false;                // this context has (or simulates) strip faces
    bool faces = false;                 // ... and at least one of them is an internal face
    bool tune = true, can_tune = true;  // option "tune"; the grid is neither too small nor too large to measure
    bool no_tall = false;               // the collision model has no tall fp32 regions (collision_models: no such instantiation of them)
    bool park = false;                  // contracted arithmetic of a model that has the tall fp64 regions (collision_models)
};

// The strip rule: 0: three iterations on 64x12 LDS tiles in pairs between exchanges; 1: six iterations on 64x16 LDS tiles of
// 1024 threads (one cell per thread: the shortest launch, and on strips this short the chain edge band -> exchange -> edge band IS
// the time step); 7: six iterations on 64x32 regions held in registers (four cells per thread: the highest throughput).
// One GPU, one rank of N exchanging with itself through RCCL, 4096 columns (tools/strip_proxy.py, profiles/r03): 128 rows
// 7.6 us per iteration on the LDS tiles against 8.5 in registers; 256 rows 13.2 against 11.6. A function of the GLOBAL grid and
// the number of strips only: every rank — measuring or not — issues the same launch depths.
inline int strip_rule_deep(bool strips, int ny_glob, int nstrips) {
    const int strip_rows = ny_glob / (nstrips > 0 ? nstrips : 1);
    return !strips ? 0 : strip_rows >= 192 ? DEEP_COL6 : strip_rows >= 64 ? DEEP_LDS6 : 0;
}

// Every candidate lbm_initialise times for this context (one entry: nothing is measured). `fixed` = the plan the options pin.
inline std::vector<Plan> plan_candidates(const PlanQuery& q, const Plan& fixed) {
    std::vector<Plan> cand;
    // "small": 1024-cell tiles make at most two rounds of one block per CU (fp32: two blocks per CU)
    const bool small_grid = (size_t)q.nx * q.nyl <= (size_t)2048 * q.num_cus * (q.esize == 4 ? 2 : 1);
    const int strip_deep = strip_rule_deep(q.strips, q.ny_glob, q.nstrips);
    const std::string deep_name = deep_is_col(strip_deep) ? "row-interleaved/6-step 64x32 in registers" : "row-interleaved/6-step 64x16";
    if (!q.tune) { cand.push_back(fixed); return cand; }
    if (!q.can_tune) {
        if (strip_deep) cand.push_back({1, 1, 0, 6, 12, 1, deep_name + " (default, not measured)", strip_deep});
        else if (q.strips) cand.push_back({1, 1, 0, 3, 12, 1, "row-interleaved (default, not measured)"});
        else cand.push_back({0, 1, 0, 3, 12, 0, "planar (default, not measured)"});
        return cand;
    }
    // Strips exchange GR rows x 9 sub-rows as one contiguous run: row-interleaved only. Every rank must issue the same
    // sequence of launches (one exchange per launch), so the fusion depth and tile shape of a strip run are fixed by rule;
    // only rank-local choices (the store policy) are measured.
    if (strip_deep) {
        cand.push_back({1, 1, 0, 6, 12, 1, deep_name + "/nt-store/xcd", strip_deep});
        cand.push_back({1, 0, 0, 6, 12, 1, deep_name + "/xcd", strip_deep});
        if (deep_is_col(strip_deep)) cand.push_back({1, 0, 0, 6, 12, 1, deep_name + "/nt-load/xcd", strip_deep, 1});
        return cand;
    }
    if (q.strips) {
        cand.push_back({1, 1, 0, 3, 12, 1, "row-interleaved/3-step 64x12/nt-store/xcd"});
        cand.push_back({1, 1, 0, 3, 12, 0, "row-interleaved/3-step 64x12/nt-store"});
        cand.push_back({1, 0, 1, 3, 12, 1, "row-interleaved/3-step 64x12/alternate/xcd"});
        return cand;
    }
    cand.push_back({1, 1, 0, 4, 8, 1, "row-interleaved/4-step 64x8/nt-store/xcd"});
    cand.push_back({1, 1, 0, 6, 12, 1, "row-interleaved/6-step 64x32 in registers/nt-store/xcd", 7});   // k_stepc_col
    cand.push_back({1, 1, 0, 5, 12, 1, "row-interleaved/5-step 64x32 in registers/nt-store/xcd", 6});
    // (non-temporal stores pay where most of the lattice fits the 256 MiB Infinity Cache — 4096x1024 fp64: +1 % — and
    // cost 3-12 % on the large grids: 8192x2048 fp64 168 -> 173 GLUPS, 16384x4096 fp32 259 -> 290 without them)
    cand.push_back({1, 0, 0, 6, 12, 1, "row-interleaved/6-step 64x32 in registers/xcd", 7});
    cand.push_back({1, 0, 0, 5, 12, 1, "row-interleaved/5-step 64x32 in registers/xcd", 6});
    cand.push_back({1, 0, 1, 6, 12, 1, "row-interleaved/6-step 64x32 in registers/alternate/xcd", 7});
    // (round 4: non-temporal level-1 LOADS with plain stores: 164-167 against 158-163 GLUPS at 4096x1024 fp64)
    cand.push_back({1, 0, 0, 6, 12, 1, "row-interleaved/6-step 64x32 in registers/nt-load/xcd", 7, 1});
    cand.push_back({1, 0, 1, 6, 12, 1, "row-interleaved/6-step 64x32 in registers/nt-load/alternate/xcd", 7, 1});
    cand.push_back({1, 0, 0, 5, 12, 1, "row-interleaved/5-step 64x32 in registers/nt-load/xcd", 6, 1});
    // (round 4: seven iterations as the plan's own depth pay on the largest grids — 8192x2048 fp64 175.9 GLUPS against 169.9 for six;
    // at 4096x1024 they lose, 157-160 against 160-166)
    if (!small_grid) {
        cand.push_back({1, 0, 0, 7, 12, 1, "row-interleaved/7-step 64x32 in registers/xcd", 9});
        cand.push_back({1, 0, 1, 7, 12, 1, "row-interleaved/7-step 64x32 in registers/alternate/xcd", 9});
    }
    // (round 4, fp32: 64x48 regions on twelve waves — 16384x4096 320 GLUPS against 289-298 on 64x32; 4096x1024 262 against 260)
    if (q.esize == 4 && !small_grid && !q.no_tall) {
        cand.push_back({1, 0, 0, 7, 12, 1, "row-interleaved/7-step 64x48 in registers/xcd", 8});
        cand.push_back({1, 0, 1, 7, 12, 1, "row-interleaved/7-step 64x48 in registers/alternate/xcd", 8});
    }
    // (fp64 contracted: 64x40 regions, the fifth row parked in LDS. tools/colbench, 4096x1024: seven iterations with non-temporal loads
    // 24.8 us per iteration against 26.0 for the best 64x32 form; six iterations LOSE there, 26.2-27.5 against 26.0, a launch being 5.2
    // rounds of blocks — they are measured because "split" hides a short last round; profiles/col_parked/README.md. Where a six-iteration
    // launch on 64x32 regions is at least six rounds of blocks, two per CU.)
    if (q.esize == 8 && q.park && (long)((q.nx + 53) / 54) * ((q.nyl + 21) / 22) >= 6L * 2 * q.num_cus) {
        cand.push_back({1, 0, 1, 6, 12, 1, "row-interleaved/6-step 64x40 in registers/nt-load/alternate/xcd", 10, 1});
        cand.push_back({1, 0, 0, 6, 12, 1, "row-interleaved/6-step 64x40 in registers/nt-load/xcd", 10, 1});
        cand.push_back({1, 0, 1, 6, 12, 1, "row-interleaved/6-step 64x40 in registers/alternate/xcd", 10});
        cand.push_back({1, 1, 0, 6, 12, 1, "row-interleaved/6-step 64x40 in registers/nt-store/xcd", 10});
        cand.push_back({1, 0, 1, 7, 12, 1, "row-interleaved/7-step 64x40 in registers/alternate/xcd", 11});
        cand.push_back({1, 0, 0, 7, 12, 1, "row-interleaved/7-step 64x40 in registers/nt-load/xcd", 11, 1});
        cand.push_back({1, 0, 1, 7, 12, 1, "row-interleaved/7-step 64x40 in registers/nt-load/alternate/xcd", 11, 1});
    }
    cand.push_back({1, 1, 0, 6, 12, 1, "row-interleaved/6-step 64x16/nt-store/xcd", 1});
    if (small_grid && !q.faces) {   // one round of LDS-filling tiles: a launch's load and store phases are paid once per 7-8 iterations
        cand.push_back({1, 1, 0, 7, 12, 1, "row-interleaved/7-step 64x16/nt-store/xcd", 2});
        cand.push_back({1, 1, 0, 8, 12, 1, "row-interleaved/8-step 32x32/nt-store/xcd", 3});
    }
    cand.push_back({1, 1, 0, 3, 12, 1, "row-interleaved/3-step 64x12/nt-store/xcd"});
    cand.push_back({1, 1, 0, 3, 8, 1, "row-interleaved/3-step 64x8/nt-store/xcd"});
    cand.push_back({1, 1, 0, 2, 12, 1, "row-interleaved/2-step 64x12/nt-store/xcd"});
    cand.push_back({1, 1, 0, 2, 8, 1, "row-interleaved/2-step 64x8/nt-store/xcd"});
    cand.push_back({1, 1, 0, 1, 0, 0, "row-interleaved/site/nt-store"});
    cand.push_back({1, 0, 1, 1, 0, 0, "row-interleaved/site/alternate"});
    cand.push_back({0, 1, 0, 4, 8, 1, "planar/4-step 64x8/nt-store/xcd"});
    cand.push_back({0, 1, 0, 6, 12, 1, "planar/6-step 64x32 in registers/nt-store/xcd", 7});
    cand.push_back({0, 1, 0, 3, 12, 1, "planar/3-step 64x12/nt-store/xcd"});
    cand.push_back({0, 1, 0, 3, 12, 0, "planar/3-step 64x12/nt-store"});
    cand.push_back({0, 1, 0, 2, 12, 0, "planar/2-step 64x12/nt-store"});
    cand.push_back({0, 0, 1, 3, 12, 0, "planar/3-step 64x12/alternate"});
    cand.push_back({0, 0, 1, 1, 0, 0, "planar/site/alternate"});
    return cand;
}

// the dominant kernel of a plan, as rocprofv3 names it (minus "lbmk::" and blanks)
// (arith: the kernels' Arith value, 0..5, 8, 9, 16, 17, 32, 33; the region shapes follow its strict / contracted half; the store policy is the row's)
inline std::string plan_kernel_name(int fuse, int deep, int pair_ty, int nt, int arith, int esize) {
    char name[96];
    const char* t = esize == 4 ? "float" : "double";
    const RegionKind* k = deep_kind(deep);
    const RowsWaves rw = k ? col_rw(*k, esize, arith & 1) : RowsWaves{};
    const char* nts = nt && (!k || col_depth(*k, deep_depth(deep))->nt) ? "true" : "false";
    if (fuse > 2 && k) snprintf(name, sizeof(name), "k_stepc_col<%s,%d,%d,%d,%s,%d>", t, rw.rows, rw.waves, deep_depth(deep), nts, arith);
    else if (fuse > 2 && deep) snprintf(name, sizeof(name), "k_stepd_tile<%s,%d,%d,%d,%d>", t, deep_shape(deep)->tile_w, deep_shape(deep)->tile_h, deep_depth(deep), arith);
    else if (fuse == 4) snprintf(name, sizeof(name), "k_step4_tile<%s,8,%d,%d>", t, esize == 8 ? 1024 : 512, arith);
    else if (fuse > 1) snprintf(name, sizeof(name), "k_step%d_tile<%s,%d,%d,%d>", fuse, t, pair_ty, pair_ty == 12 ? (fuse == 3 ? 1024 : 768) : 512, arith);
    else snprintf(name, sizeof(name), "k_step_site<%s,0,%s,%d>", t, nts, arith);
    return name;
}

// the plan as lbm_set_option pairs: `deep` (which sets the depth of its launches itself) or `fuse`, never both
inline std::string plan_option_string(int layout, int nt, int alternate, int pair_ty, int xcd, int fuse, int deep, int ntl = 0) {
    char b[128];
    snprintf(b, sizeof(b), "layout=%d nt=%d alternate=%d pair_ty=%d xcd=%d", layout, nt, alternate, pair_ty ? pair_ty : 8, xcd);
    std::string s(b);
    if (deep) s += " deep=" + std::to_string(deep);
    else s += " fuse=" + std::to_string(fuse > 0 && fuse <= 4 ? fuse : 1);
    if (ntl) s += " ntl=1";
    return s;
}

// The index arithmetic of a ring of `cap` slots that is filled at the output iterations of lbm_step and drained oldest first (the
// two force logs, the frame ring, the probe ring: DeviceRing, lbm_ctx.hpp). The only place that wraps an index; exported through
// lbm_debug_ring (tests/test_ring_cpu.py holds it against a deque).
struct RingIndex {
    int cap = 0, head = 0, count = 0;
    void reset() { head = count = 0; }                     // forget what is pending
    bool full() const { return count >= cap; }
    int next() const { return (head + count) % cap; }      // the slot of the next sample (not full, so cap > 0)
    void commit() { ++count; }                             // ... once it has been queued
    // up to `m` of the oldest samples: slots [start, start + n1), then [0, n2)
    struct Span { int start, n1, n2; };
    Span oldest(int m) const {
        const int n = m < 0 ? 0 : m < count ? m : count;
        const int n1 = n < cap - head ? n : cap - head;
        return {head, n1, n - n1};
    }
    void drop(int n) { if (n > 0) { head = (head + n) % cap; count -= n; } }      // (n <= count, as `oldest` counted them)
};

}  // namespace lbmk
