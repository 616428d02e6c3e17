// csrc/lbm_col.hip — the translation unit(s) of k_stepc_col (lbm_kernel_col.hpp) and the launchers lbm_hip.hip calls (lbm_col_api.hpp).
// -DLBM_COL_T=<element type> -DLBM_AR_BASE=<a collision model's Arith base>: the ten instantiations of that type and model on 64 x 32
// regions (five / six iterations x store policy + seven iterations, x arithmetic); -DLBM_COL_TALL=1 / 0: the three tall fp32 ones of
// one arithmetic mode, BGK only; -DLBM_COL_PARK=<base>: the five of the tall fp64 regions (64 x 40, contracted) of one model. One object
// each (build.py). The forced model (base 8) is named by -DLBM_AR_FORCED_BASE=8 / -DLBM_COL_FORCED_PARK=8 instead.
#include "lbm_kernel_col.hpp"
#include "lbm_col_api.hpp"

#if !defined(LBM_AR_BASE) && defined(LBM_AR_FORCED_BASE)    // the forced model's objects carry flags of their own (build.py FORCED_BASES)
#define LBM_AR_BASE LBM_AR_FORCED_BASE
#endif
#if !defined(LBM_COL_PARK) && defined(LBM_COL_FORCED_PARK)
#define LBM_COL_PARK LBM_COL_FORCED_PARK
#endif

namespace lbmk {

#define LBM_KC(T_, D_, R_, NW_, NT_, AR_) do { \
        constexpr int OW_ = col_tile_w(D_), OH_ = col_tile_h(D_, R_, NW_); \
        const int nb_ = ((a.nx + OW_ - 1) / OW_) * ((a.y_cnt + OH_ - 1) / OH_ + (a.y_cnt2 + OH_ - 1) / OH_); \
        const dim3 gridc((unsigned)((nb_ + 7) / 8 * 8)), blockc(NW_ * 64); \
        hipLaunchKernelGGL((k_stepc_col<T_, R_, NW_, D_, NT_, AR_>), gridc, blockc, 0, s, a, e); } while (0)

#if defined(LBM_COL_T) && defined(LBM_AR_BASE)   // the 64 x 32 (fp64 strict: 64 x 24 on twelve waves) regions of one element type and model
template <typename T, int ARB>
void launch_col(const KArgs<T>& a, const K2Extra<T>& e, int depth, bool nt, bool contracted, hipStream_t s) {
    constexpr int ARS = ARB, ARC = ARB | 1;
#define LBM_KD(D_) do { \
        if (contracted) { if (nt) LBM_KC(T, D_, RC, WC, true, ARC); else LBM_KC(T, D_, RC, WC, false, ARC); } \
        else { if (nt) LBM_KC(T, D_, RS, WS, true, ARS); else LBM_KC(T, D_, RS, WS, false, ARS); } } while (0)
    constexpr int RC = col_rows_per_thread((int)sizeof(T), false), RS = col_rows_per_thread((int)sizeof(T), true);
    constexpr int WC = col_waves((int)sizeof(T), false), WS = col_waves((int)sizeof(T), true);
    // (seven iterations: plain stores only — the depth of a call's remainders and of the "deep" 9 plans, whose candidates all store plainly)
    if (depth == 5) LBM_KD(5);
    else if (depth == 7) { if (contracted) LBM_KC(T, 7, RC, WC, false, ARC); else LBM_KC(T, 7, RS, WS, false, ARS); }
    else LBM_KD(6);
#undef LBM_KD
}
template void launch_col<LBM_COL_T, LBM_AR_BASE>(const KArgs<LBM_COL_T>&, const K2Extra<LBM_COL_T>&, int, bool, bool, hipStream_t);
#elif defined(LBM_COL_TALL)  // the tall fp32 regions (64 x 48) of one arithmetic mode: contracted 12 waves x 4 rows (1), strict 8 x 6 (0)
#if LBM_COL_TALL
void launch_col_tall_contracted(const KArgs<float>& a, const K2Extra<float>& e, int depth, hipStream_t s) {
    constexpr int R = col_rows_per_thread(4, false, true), W = col_waves(4, false, true), AR = AR_CONTRACTED;
#else
void launch_col_tall_strict(const KArgs<float>& a, const K2Extra<float>& e, int depth, hipStream_t s) {
    constexpr int R = col_rows_per_thread(4, true, true), W = col_waves(4, true, true), AR = AR_STRICT;
#endif
    if (depth == 6) LBM_KC(float, 6, R, W, false, AR); else if (depth == 8) LBM_KC(float, 8, R, W, false, AR); else LBM_KC(float, 7, R, W, false, AR);
}
#elif defined(LBM_COL_PARK)  // the tall fp64 regions (64 x 40, eight waves x five rows, the top row parked in LDS), contracted, of one model
template <int ARB>
void launch_col_park(const KArgs<double>& a, const K2Extra<double>& e, int depth, bool nt, hipStream_t s) {
    constexpr int R = col_rows_per_thread(8, false, true), W = col_waves(8, false, true), AR = ARB | 1;
    if (depth == 5) { if (nt) LBM_KC(double, 5, R, W, true, AR); else LBM_KC(double, 5, R, W, false, AR); }
    else if (depth == 7) LBM_KC(double, 7, R, W, false, AR);
    else { if (nt) LBM_KC(double, 6, R, W, true, AR); else LBM_KC(double, 6, R, W, false, AR); }
}
template void launch_col_park<LBM_COL_PARK>(const KArgs<double>&, const K2Extra<double>&, int, bool, hipStream_t);
#else
#error "compile with -DLBM_COL_T=double or float and -DLBM_AR_BASE=0, 2 or 4 (a collision model's Arith base), with -DLBM_COL_TALL=1 or 0, or with -DLBM_COL_PARK=<base>"
#endif
#undef LBM_KC

}  // namespace lbmk
