// csrc/lbm_col.hip — the translation unit(s) of k_stepc_col (lbm_kernel_col.hpp) and the launcher lbm_hip.hip calls (lbm_col_api.hpp).
// An object holds the kernels of ONE region kind (region_kinds, lbm_plan.hpp), exactly the (depth, store policy) pairs its row lists:
// -DLBM_COL_T=<element type> -DLBM_AR_BASE=<a collision model's Arith base>: the 64 x 32 regions of that type and model, both arithmetic
// modes (ten kernels); -DLBM_COL_TALL=1 / 0: the fp32 64 x 48 regions of one arithmetic mode, BGK only (eight unrolled rows x up to eight
// levels compile slowly); -DLBM_COL_PARK=<base>: the fp64 64 x 40 regions of one model, contracted. One object each (build.py).
#include "lbm_kernel_col.hpp"
#include "lbm_col_api.hpp"

namespace lbmk {

template <typename T, int KIND, int AR>
bool launch_col(const KArgs<T>& a, const K2Extra<T>& e, int depth, bool nt, hipStream_t s) {
    static_assert(col_built<T, KIND, AR>());
    constexpr RowsWaves RW = col_rw(region_kinds[KIND], (int)sizeof(T), AR & 1);
    return with_row<std::size(region_kinds[KIND].depths)>([&](size_t i) { return region_kinds[KIND].depths[i].depth == depth; }, [&](auto i) {
        constexpr ColDepth D = region_kinds[KIND].depths[i()];
        constexpr int OW = col_tile_w(D.depth), OH = col_tile_h(D.depth, RW);
        const int nb = ((a.nx + OW - 1) / OW) * ((a.y_cnt + OH - 1) / OH + (a.y_cnt2 + OH - 1) / OH);
        const dim3 grid((unsigned)((nb + 7) / 8 * 8)), block(RW.waves * 64);
        if constexpr (D.nt) { if (nt) { hipLaunchKernelGGL((k_stepc_col<T, RW.rows, RW.waves, D.depth, true, AR>), grid, block, 0, s, a, e); return; } }
        hipLaunchKernelGGL((k_stepc_col<T, RW.rows, RW.waves, D.depth, false, AR>), grid, block, 0, s, a, e);
    });
}
#define LBM_COL_INST(T_, KIND_, AR_) template bool launch_col<T_, KIND_, AR_>(const KArgs<T_>&, const K2Extra<T_>&, int, bool, hipStream_t)
#if defined(LBM_COL_T) && defined(LBM_AR_BASE)
LBM_COL_INST(LBM_COL_T, RK_STD, LBM_AR_BASE);
LBM_COL_INST(LBM_COL_T, RK_STD, LBM_AR_BASE | 1);
#if LBM_AR_BASE == 4      // TRT's objects hold the model that rides with it (collision_models: unit), MRT
static_assert(LBM_AR_BASE == AR_STRICT_TRT && collision_model(AR_STRICT_MRT).unit == AR_STRICT_TRT);
LBM_COL_INST(LBM_COL_T, RK_STD, AR_STRICT_MRT);
LBM_COL_INST(LBM_COL_T, RK_STD, AR_STRICT_MRT | 1);
#endif
#if LBM_AR_BASE == 0      // ... and BGK's the outlet sponge
static_assert(LBM_AR_BASE == AR_STRICT && collision_model(AR_STRICT_SPONGE).unit == AR_STRICT);
LBM_COL_INST(LBM_COL_T, RK_STD, AR_STRICT_SPONGE);
LBM_COL_INST(LBM_COL_T, RK_STD, AR_STRICT_SPONGE | 1);
#endif
#elif defined(LBM_COL_TALL)
LBM_COL_INST(float, RK_TALL, AR_STRICT | LBM_COL_TALL);
#elif defined(LBM_COL_PARK)
LBM_COL_INST(double, RK_PARK, LBM_COL_PARK | 1);
#else
#error "compile with -DLBM_COL_T=double or float and -DLBM_AR_BASE=<a collision model's Arith base>, with -DLBM_COL_TALL=1 or 0, or with -DLBM_COL_PARK=<base>"
#endif
#undef LBM_COL_INST

}  // namespace lbmk
