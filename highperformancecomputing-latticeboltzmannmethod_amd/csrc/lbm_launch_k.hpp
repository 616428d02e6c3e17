// csrc/lbm_launch_k.hpp — the kernel launches of the single-iteration and fused tile families for one pair of arithmetic values
// (ARS strict, ARC contracted): AR_STRICT / AR_CONTRACTED in lbm_hip.hip (BGK), AR_STRICT_LES / AR_CONTRACTED_LES in lbm_les.hip
// (Smagorinsky), AR_STRICT_TRT / AR_CONTRACTED_TRT in lbm_trt.hip (two relaxation times). A template is instantiated where it is used, so each translation unit holds the kernels of its own pair only.
#pragma once
#include "lbm_kernels.hpp"

namespace lbmk {

// k_step_site over the rows a.y_lo.. / a.y_lo2.. of the launch: MODE_STEP in both store policies, MODE_COLLIDE_ONLY plain, MODE_STREAM_ONLY
// (no collision in it) with ARS
template <typename T, int MODE, int ARS, int ARC>
void launch_site_k(const KArgs<T>& a, bool nt, bool fast, hipStream_t s) {
    const dim3 grid((a.nx + 255) / 256, a.y_cnt + a.y_cnt2), block(256);
#define LBM_K1(NT_, AR_) hipLaunchKernelGGL((k_step_site<T, MODE, NT_, AR_>), grid, block, 0, s, a)
    if constexpr (MODE == MODE_STEP) {
        if (fast) { if (nt) LBM_K1(true, ARC); else LBM_K1(false, ARC); }
        else { if (nt) LBM_K1(true, ARS); else LBM_K1(false, ARS); }
    } else if constexpr (MODE == MODE_COLLIDE_ONLY) {
        if (fast) LBM_K1(false, ARC); else LBM_K1(false, ARS);
    } else {
        LBM_K1(false, ARS);
    }
#undef LBM_K1
}

// k_stepd_tile on LDS shape `shape` (1: 64x16 six iterations, 2: 64x16 seven, 3: 32x32 eight)
template <typename T, int ARS, int ARC>
void launch_deep_k(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s) {
#define LBM_KD(TX_, TY_, D_) do { \
        dim3 gridd((a.nx + TX_ - 1) / TX_, (a.y_cnt + TY_ - 1) / TY_ + (a.y_cnt2 + TY_ - 1) / TY_); \
        if (fast) hipLaunchKernelGGL((k_stepd_tile<T, TX_, TY_, D_, ARC>), gridd, dim3(TX_ * TY_), 0, s, a, e); \
        else hipLaunchKernelGGL((k_stepd_tile<T, TX_, TY_, D_, ARS>), gridd, dim3(TX_ * TY_), 0, s, a, e); } while (0)
    switch (shape) {
        case 1: LBM_KD(64, 16, 6); break;
        case 2: LBM_KD(64, 16, 7); break;
        default: LBM_KD(32, 32, 8); break;
    }
#undef LBM_KD
}

// k_step2/3/4_tile: `depth` iterations on bands of `ty` rows (depth 4: 64x8 tiles only)
template <typename T, int ARS, int ARC>
void launch_tile_k(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s) {
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

// ---- the LES instantiations (lbm_les.hip; k_stepc_col's: lbm_col.hip -DLBM_COL_LES=1) -----------------------------------------
// mode: MODE_STEP or MODE_COLLIDE_ONLY
template <typename T>
void launch_site_les(const KArgs<T>& a, int mode, bool nt, bool fast, hipStream_t s);
template <typename T>
void launch_deep_les(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s);
template <typename T>
void launch_tile_les(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s);

// ---- the TRT instantiations (lbm_trt.hip; k_stepc_col's: lbm_col.hip -DLBM_COL_TRT=1) -----------------------------------------
template <typename T>
void launch_site_trt(const KArgs<T>& a, int mode, bool nt, bool fast, hipStream_t s);
template <typename T>
void launch_deep_trt(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s);
template <typename T>
void launch_tile_trt(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s);

}  // namespace lbmk
