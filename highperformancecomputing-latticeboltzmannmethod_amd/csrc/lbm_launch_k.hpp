// csrc/lbm_launch_k.hpp — what the host translation unit (lbm_hip.hip) sees of the single-iteration and fused tile families: one launcher
// per family, over the element type and the collision model's Arith base ARB (collision_models, lbm_plan.hpp; the kernels run ARB strict
// or ARB | 1 contracted). Declared only: lbm_step_k.hip defines them and instantiates them explicitly, once per base (-DLBM_AR_BASE,
// build.py), so no other translation unit can instantiate a step kernel.
#pragma once
#include "lbm_plan.hpp"

namespace lbmk {

// k_step_site over the rows a.y_lo.. / a.y_lo2.. of the launch: MODE_STEP in both store policies, MODE_COLLIDE_ONLY plain, and under
// AR_STRICT alone MODE_STREAM_ONLY (no collision in it)
template <typename T, int ARB>
void launch_site(const KArgs<T>& a, int mode, bool nt, bool fast, hipStream_t s);
// k_stepd_tile on the tile and with the depth of the LDS row `shape` of deep_shapes (lbm_plan.hpp); false, and nothing queued: no such row
template <typename T, int ARB>
bool launch_deep(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s);
// k_step2/3/4_tile: `depth` iterations on bands of `ty` rows (depth 4: 64x8 tiles only)
template <typename T, int ARB>
void launch_tile(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s);

}  // namespace lbmk
