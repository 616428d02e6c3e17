// csrc/lbm_step_k.hip — the single-iteration and fused tile kernel families (k_step_site, k_step2/3/4_tile, k_stepd_tile) of ONE collision
// model and their launchers (lbm_launch_k.hpp), for both element types: compiled once per model with -DLBM_AR_BASE=<the model's Arith
// base> (build.py), side by side with the host translation unit. MODE_STREAM_ONLY has no collision in it: base 0 alone holds it.
#include "lbm_launch_k.hpp"

#ifndef LBM_AR_BASE
#error "compile with -DLBM_AR_BASE=<Arith base of a collision model that has objects of its own: 0, 2, 4 or 8>"
#endif

namespace lbmk {

template <typename T, int ARB>
void launch_site(const KArgs<T>& a, int mode, bool nt, bool fast, hipStream_t s) {
    constexpr int ARS = ARB, ARC = ARB | 1;
    const dim3 grid((a.nx + 255) / 256, a.y_cnt + a.y_cnt2), block(256);
#define LBM_K1(MODE_, NT_, AR_) hipLaunchKernelGGL((k_step_site<T, MODE_, NT_, AR_>), grid, block, 0, s, a)
    if (mode == MODE_STEP) {
        if (fast) { if (nt) LBM_K1(MODE_STEP, true, ARC); else LBM_K1(MODE_STEP, false, ARC); }
        else { if (nt) LBM_K1(MODE_STEP, true, ARS); else LBM_K1(MODE_STEP, false, ARS); }
    } else if (mode == MODE_COLLIDE_ONLY) {
        if (fast) LBM_K1(MODE_COLLIDE_ONLY, false, ARC); else LBM_K1(MODE_COLLIDE_ONLY, false, ARS);
    } else if constexpr (ARB == AR_STRICT) {
        LBM_K1(MODE_STREAM_ONLY, false, ARS);
    }
#undef LBM_K1
}

template <typename T, int ARB>
bool launch_deep(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s) {
    return with_row<std::size(deep_shapes)>([&](size_t i) { return deep_shapes[i].id == shape && deep_shapes[i].kind < 0; }, [&](auto i) {
        constexpr DeepShape S = deep_shapes[i()];
        if constexpr (S.kind < 0) {
            constexpr int TX = S.tile_w, TY = S.tile_h;
            dim3 gridd((a.nx + TX - 1) / TX, (a.y_cnt + TY - 1) / TY + (a.y_cnt2 + TY - 1) / TY);
            if (fast) hipLaunchKernelGGL((k_stepd_tile<T, TX, TY, S.depth, ARB | 1>), gridd, dim3(TX * TY), 0, s, a, e);
            else hipLaunchKernelGGL((k_stepd_tile<T, TX, TY, S.depth, ARB>), gridd, dim3(TX * TY), 0, s, a, e);
        }
    });
}

template <typename T, int ARB>
void launch_tile(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s) {
    constexpr int ARS = ARB, ARC = ARB | 1;
    dim3 grid((a.nx + 63) / 64, (a.y_cnt + ty - 1) / ty + (a.y_cnt2 + ty - 1) / ty);
#define LBM_KT(K_, TY_, NTH_, G_) do { if (fast) hipLaunchKernelGGL((K_<T, TY_, NTH_, ARC>), G_, dim3(NTH_), 0, s, a, e); \
                                       else hipLaunchKernelGGL((K_<T, TY_, NTH_, ARS>), G_, dim3(NTH_), 0, s, a, e); } while (0)
    if (depth == 4) {   // four iterations: 64x8 tiles only (LDS)
        dim3 grid4((a.nx + 63) / 64, (a.y_cnt + 7) / 8 + (a.y_cnt2 + 7) / 8);
        // fp64: 70.5 KB of LDS per block = two blocks per CU, so 1024 threads fill the 32 wave slots; fp32 (35 KB) fills them
        // with four 512-thread blocks (measured: 1024 threads -14 % in fp32, +3 % in fp64)
        constexpr int N4 = sizeof(T) == 8 ? 1024 : 512;
        LBM_KT(k_step4_tile, 8, N4, grid4);
    } else if (depth == 3) {
        if (ty == 12) LBM_KT(k_step3_tile, 12, 1024, grid); else LBM_KT(k_step3_tile, 8, 512, grid);
    } else {
        if (ty == 12) LBM_KT(k_step2_tile, 12, 768, grid); else LBM_KT(k_step2_tile, 8, 512, grid);
    }
#undef LBM_KT
}

#define LBM_STEP_K_INST(T_, ARB_) \
    template void launch_site<T_, ARB_>(const KArgs<T_>&, int, bool, bool, hipStream_t); \
    template bool launch_deep<T_, ARB_>(const KArgs<T_>&, const K2Extra<T_>&, int, bool, hipStream_t); \
    template void launch_tile<T_, ARB_>(const KArgs<T_>&, const K2Extra<T_>&, int, int, bool, hipStream_t);
LBM_STEP_K_INST(double, LBM_AR_BASE)
LBM_STEP_K_INST(float, LBM_AR_BASE)
#if LBM_AR_BASE == 4      // TRT's objects hold the model that rides with it (collision_models: unit), MRT
static_assert(LBM_AR_BASE == AR_STRICT_TRT && collision_model(AR_STRICT_MRT).unit == AR_STRICT_TRT);
LBM_STEP_K_INST(double, AR_STRICT_MRT)
LBM_STEP_K_INST(float, AR_STRICT_MRT)
#endif
#if LBM_AR_BASE == 0      // ... and BGK's the outlet sponge
static_assert(LBM_AR_BASE == AR_STRICT && collision_model(AR_STRICT_SPONGE).unit == AR_STRICT);
LBM_STEP_K_INST(double, AR_STRICT_SPONGE)
LBM_STEP_K_INST(float, AR_STRICT_SPONGE)
#endif
#undef LBM_STEP_K_INST

}  // namespace lbmk
