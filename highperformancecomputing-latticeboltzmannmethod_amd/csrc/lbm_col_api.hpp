// csrc/lbm_col_api.hpp — what the host translation unit (lbm_hip.hip) sees of the register-resident column kernel: its launcher.
// The region shapes are the rows of region_kinds (lbm_plan.hpp). The kernel itself (lbm_kernel_col.hpp) is compiled in its own
// translation unit (lbm_col.hip) so that the two halves of the device code build side by side (build.py).
#pragma once
#include "lbm_plan.hpp"

namespace lbmk {

// does the library hold k_stepc_col on regions of kind KIND for element type T and Arith value AR?
template <typename T, int KIND, int AR>
constexpr bool col_built() {
    constexpr const RegionKind& k = region_kinds[KIND];
    return col_rw(k, (int)sizeof(T), AR & 1).rows && (!k.needs || collision_model(AR).*k.needs);
}
// k_stepc_col<T, rows per thread, waves, depth, nt, AR> over the rows a.y_lo.. / a.y_lo2.. of the launch, `depth` one of the kind's; nt
// counts where the depth's row has such an instantiation. false, and nothing queued: the kind does not offer the depth.
// Declared only: lbm_col.hip defines it and instantiates it explicitly where col_built says so — one object file per element type and
// model for RK_STD, per arithmetic mode for RK_TALL, per model for RK_PARK — so no other translation unit can instantiate the kernel.
template <typename T, int KIND, int AR>
bool launch_col(const KArgs<T>& a, const K2Extra<T>& e, int depth, bool nt, hipStream_t s);

}  // namespace lbmk
