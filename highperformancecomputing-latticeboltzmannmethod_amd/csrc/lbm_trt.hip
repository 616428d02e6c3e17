// csrc/lbm_trt.hip — the two-relaxation-time (TRT) instantiations of the site and tile kernel families (k_step_site in MODE_STEP and
// MODE_COLLIDE_ONLY, k_step2/3/4_tile, k_stepd_tile) with AR_STRICT_TRT / AR_CONTRACTED_TRT, for both element types. A translation
// unit of their own (build.py), so that they compile beside lbm_hip.hip, whose BGK kernels they leave untouched.
#include "lbm_launch_k.hpp"

namespace lbmk {

template <typename T>
void launch_site_trt(const KArgs<T>& a, int mode, bool nt, bool fast, hipStream_t s) {
    if (mode == MODE_COLLIDE_ONLY) launch_site_k<T, MODE_COLLIDE_ONLY, AR_STRICT_TRT, AR_CONTRACTED_TRT>(a, false, fast, s);
    else launch_site_k<T, MODE_STEP, AR_STRICT_TRT, AR_CONTRACTED_TRT>(a, nt, fast, s);
}
template <typename T>
void launch_deep_trt(const KArgs<T>& a, const K2Extra<T>& e, int shape, bool fast, hipStream_t s) {
    launch_deep_k<T, AR_STRICT_TRT, AR_CONTRACTED_TRT>(a, e, shape, fast, s);
}
template <typename T>
void launch_tile_trt(const KArgs<T>& a, const K2Extra<T>& e, int depth, int ty, bool fast, hipStream_t s) {
    launch_tile_k<T, AR_STRICT_TRT, AR_CONTRACTED_TRT>(a, e, depth, ty, fast, s);
}

#define LBM_TRT_INST(T_) \
    template void launch_site_trt<T_>(const KArgs<T_>&, int, bool, bool, hipStream_t); \
    template void launch_deep_trt<T_>(const KArgs<T_>&, const K2Extra<T_>&, int, bool, hipStream_t); \
    template void launch_tile_trt<T_>(const KArgs<T_>&, const K2Extra<T_>&, int, int, bool, hipStream_t);
LBM_TRT_INST(double)
LBM_TRT_INST(float)
#undef LBM_TRT_INST

}  // namespace lbmk
