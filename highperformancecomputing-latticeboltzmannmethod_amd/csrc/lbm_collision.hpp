// csrc/lbm_collision.hpp — the collision of the step kernels: one operator per model and arithmetic mode, the launch-uniform values of
// each model under their own names with the one map of those names to the slots of KArgs, and collide(), which picks by Arith.
// (part of lbm_kernels.hpp, which includes it behind KArgs; nothing else includes it)
//   arithmetic     fma_t, recip_t, sqrt_t / sqrt_c, strict_div2
//   values         BgkK, LesK, TrtK, ForcedK, MrtK: what a model reads per launch; *_values forms them on the host
//   slot map       *_k (KArgs -> values, host and device) beside put (values -> KArgs, host): the only code that names a shared slot
//   strict         strict_moments, strict_eq; strict_bgk, les_tau_inv_strict, strict_trt, strict_mrt, strict_guo
//   contracted     pair_moments, contracted_velocity, contracted_eq; contracted_bgk, les_tau_inv_contracted, contracted_pairs (TRT and fp64 MRT),
//                  contracted_mrt, contracted_mrt_f32, contracted_guo
//   collide        the dispatch
#pragma once
#include <array>
#include <cmath>

namespace lbmk {

// Arithmetic of the collision (the only place the two modes differ) and its model: a kernel's Arith value is the model's base | the mode.
// Every model is a set of separate instantiations, never a runtime branch: a kernel's VGPR count is the maximum over its paths, and the
// BGK kernels have no headroom. The models exclude each other (collide's static_asserts), so of the values a bit pattern
// could name only these exist.
//   bit 0          AR_STRICT: the reference's expression tree evaluated operation by operation in IEEE arithmetic, no contraction,
//                  two IEEE divisions: bit-identical to the strict CPU oracle (library default, parity tests).
//                  AR_CONTRACTED: the same formulas as fused multiply-adds with ONE reciprocal of rho (two Newton steps on v_rcp): what
//                  the reference's own build flags permit its compiler to do (CMakeLists.txt:21-22: -ffast-math -mfma). 70 instead of
//                  150 floating-point instructions per cell; rho/u stay within 1e-10 of the reference (tests).
//   0  BGK         strict_bgk / contracted_bgk with the global rate BgkK::wp = 1/tau.
//   2  LES         (lbm_set_smagorinsky) the same two with the Smagorinsky rate of each cell: les_tau_inv_strict / les_tau_inv_contracted
//                  over LesK.
//   4  TRT         (lbm_set_trt) strict_trt / contracted_pairs over TrtK: the even part of each opposite pair relaxes with wp, the odd
//                  part with the second rate wm.
//   8  FORCED      (lbm_set_forcing) BGK under a uniform force density F, Guo's scheme, over ForcedK: the equilibrium is taken at
//                  u = (sum c f + F/2) / rho, and strict_guo / contracted_guo add the source
//                  S_i = (1 - 1/(2 tau)) w_i [3 (c_i - u) + 9 (c_i.u) c_i] . F to the relaxed populations.
//   16 MRT         (lbm_set_mrt) strict_mrt / contracted_mrt (fp32: contracted_mrt_f32) over MrtK: TRT's even and odd parts of each
//                  pair, with the even parts of the two axis pairs (and of the two diagonal pairs) split into their half sum, relaxed
//                  with the bulk rate sb like the rest population, and their half difference, relaxed with wp.
//   32 SPONGE      (lbm_set_sponge) BGK's two operators, operation for operation, with the rate of the cell's COLUMN (KArgs::wp_x,
//                  column_rate) in place of the global one.
enum Arith { AR_STRICT = 0, AR_CONTRACTED = 1, AR_STRICT_LES = 2, AR_CONTRACTED_LES = 3, AR_STRICT_TRT = 4, AR_CONTRACTED_TRT = 5,
             AR_STRICT_FORCED = 8, AR_CONTRACTED_FORCED = 9, AR_STRICT_MRT = 16, AR_CONTRACTED_MRT = 17, AR_STRICT_SPONGE = 32,
             AR_CONTRACTED_SPONGE = 33 };
constexpr bool ar_contracted(int ar) { return (ar & 1) != 0; }
constexpr bool ar_les(int ar) { return (ar & 2) != 0; }
constexpr bool ar_trt(int ar) { return (ar & 4) != 0; }
constexpr bool ar_forced(int ar) { return (ar & 8) != 0; }
constexpr bool ar_mrt(int ar) { return (ar & 16) != 0; }
constexpr bool ar_sponge(int ar) { return (ar & 32) != 0; }

__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double recip_t(double d) {      // 1/d to an ulp: v_rcp_f64 + two Newton steps
    double r = __builtin_amdgcn_rcp(d);
    r = fma_t(fma_t(-d, r, 1.0), r, r);
    r = fma_t(fma_t(-d, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ float recip_t(float d) {        // v_rcp_f32 (1 ulp) + one Newton step
    float r = __builtin_amdgcn_rcpf(d);
    return fma_t(fma_t(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ double sqrt_t(double v) { return __builtin_sqrt(v); }   // correctly rounded (rsq + refinement + scaling)
__device__ __forceinline__ float sqrt_t(float v) { return __builtin_sqrtf(v); }
// contracted arithmetic (LES): v_rsq_f64 and one Goldschmidt step, to about an ulp, for ~5 instead of ~17 instructions and fewer live
// registers (the fp64 register kernel has four spare VGPRs). Values below 1e-300, zero included, are raised to it first (rsq(0) is
// inf): a square root of 1e-150 instead of 0 beside tau^2 >= 0.25 changes nothing. fp32: v_sqrt_f32 (1 ulp).
__device__ __forceinline__ double sqrt_c(double v) {
    v = __builtin_fmax(v, 1e-300);
    const double y = __builtin_amdgcn_rsq(v);
    const double s = v * y;
    return fma_t(s, fma_t(-s, 0.5 * y, 0.5), s);
}
__device__ __forceinline__ float sqrt_c(float v) { return __builtin_amdgcn_sqrtf(v); }

// ux /= rho; uy /= rho (LBMSolver.h:108-109) in strict mode: two correctly rounded IEEE divisions by the SAME denominator.
// hipcc expands an fp64 division into v_div_scale x2, v_rcp_f64, two Newton steps on the reciprocal (four FMAs), q = a*r,
// rem = fma(-b, q, a), v_div_fmas (= fma(rem, r, q) unless the operands were scaled) and v_div_fixup (special values) — twice,
// because the scaling instruction takes the numerator too. For operands in the normal range (rho ~ 1, |rho u| < 1: nothing is
// scaled, nothing is special) the reciprocal chain depends on the denominator only, so the two divisions share it: the same
// operations on the same values in the same order => the same bits as the compiler's two expansions and as the oracle's divsd
// (every strict parity test holds the populations to np.array_equal), for 13 instead of ~26 instructions and a dozen fewer live
// registers. (A run that blows up is flagged by |f| > 1e5 long before rho or rho*u leave the range where no scaling happens.)
// RANGE of the bit-identity (tests/test_gpu_thin_spots.py::test_strict_div2_equals_ieee_division_in_its_range holds it on 4 M random
// operands through lbm_debug_strict_div2): denominators in [2^-20, 2^20], numerators 0 or of magnitude in [2^-400, 2^400] —
// populations of a stable run live in [1e-3, 1e1]. Outside it the chain is NOT an IEEE division: a -0 numerator gives +0 (the sign
// of a zero velocity is erased by the equilibrium's bracket and compares equal in every accessor), denormal quotients and
// exponent gaps beyond the fp64 range are not rescaled, rho == 0 gives NaN where IEEE gives +-inf (both flagged unstable).
__device__ __forceinline__ void strict_div2(double& a1, double& a2, double b) {
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    r = __builtin_fma(r, e, r);
    double q = a1 * r;
    a1 = __builtin_fma(__builtin_fma(-b, q, a1), r, q);
    q = a2 * r;
    a2 = __builtin_fma(__builtin_fma(-b, q, a2), r, q);
}
__device__ __forceinline__ void strict_div2(float& a1, float& a2, float b) { a1 /= b; a2 /= b; }
// test kernel (lbm_debug_strict_div2): strict_div2 beside the compiler's own IEEE divisions, element by element
template <int UNUSED = 0>      // (a template: the header is included by three translation units)
__global__ void k_debug_strict_div2(const double* a1, const double* a2, const double* b, int n, double* q1, double* q2, double* r1, double* r2) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double x = a1[k], y = a2[k];
    strict_div2(x, y, b[k]);
    q1[k] = x; q2[k] = y;
    r1[k] = a1[k] / b[k]; r2[k] = a2[k] / b[k];
}   // (fp32 has no oracle to be bit-equal to: plain divisions)

// ---- the launch-uniform values of each model, under their own names ------------------------------------------------------------------
// What a model's operators read per launch, in the element type. *_values forms them on the host from the context's tau and the model's
// parameters (lbm_ctx::collision_param, collision_param2), every value in double and cast once (a uniform value formed by the kernel
// would sit in vector registers). The outlet sponge has none: its rates are the table KArgs::wp_x.
template <typename T> struct BgkK { T wp; };                        // wp = 1/tau (LBMSolver.h:85)
template <typename T> struct LesK { T tau, tau2, c; };              // tau, tau^2, C = 18 sqrt(2) Cs^2
template <typename T> struct TrtK { T wp, wm, wa, wb; };            // wm = 1/tau_minus, (tau - 1/2)(tau_minus - 1/2) = magic; folded for the
                                                                    // contracted arithmetic: wa = (wp + wm)/2, wb = (wp - wm)/2
template <typename T> struct ForcedK { T wp, gx, gy, hx, hy; };     // Guo, Zheng and Shi 2002: g = (1 - wp/2) F, the factor of the source
                                                                    // term; h = F/2, what the equilibrium's velocity adds to the momentum
template <typename T> struct MrtK { T wp, wm, wa, wb, sb, kb; };    // TRT's four; the bulk rate sb; folded for the contracted arithmetic:
                                                                    // kb = (sb - wp)/(4 wp) = (sb tau - 1)/4
template <typename T> inline BgkK<T> bgk_values(double tau) { return {(T)(1.0 / tau)}; }
template <typename T> inline LesK<T> les_values(double tau, double cs) { return {(T)tau, (T)(tau * tau), (T)(18.0 * std::sqrt(2.0) * (cs * cs))}; }
template <typename T> inline TrtK<T> trt_values(double tau, double magic) {
    const double wp = 1.0 / tau, wm = 1.0 / (0.5 + magic / (tau - 0.5));
    return {(T)wp, (T)wm, (T)(0.5 * (wp + wm)), (T)(0.5 * (wp - wm))};
}
template <typename T> inline ForcedK<T> forced_values(double tau, double fx, double fy) {
    const double wp = 1.0 / tau, k = 1.0 - 0.5 * wp;
    return {(T)wp, (T)(k * fx), (T)(k * fy), (T)(0.5 * fx), (T)(0.5 * fy)};
}
template <typename T> inline MrtK<T> mrt_values(double tau, double sb, double magic) {
    const TrtK<T> t = trt_values<T>(tau, magic);
    return {t.wp, t.wm, t.wa, t.wb, (T)sb, (T)(0.25 * (sb * tau - 1.0))};
}

// ---- the slot map: which slot of KArgs carries which value ---------------------------------------------------------------------------
// KArgs has eight slots for these values: tau_inv, the four of the block at its front and the three unions behind `reverse`. The layout is
// pinned (the asserts behind KArgs); the names of the slots are history. Per model the reader (host and device: collide below, and
// lbm_debug_collision_args on the CPU) stands beside the writer (host: fill_collision, lbm_launch.inc.hpp). A model's kernels read its
// own slots only, which the `if constexpr` structure of collide guarantees; a context's fill leaves the others zero.
template <typename T> inline void clear_collision_slots(KArgs<T>& a) {
    a.tau_inv = a.frc_gx = a.frc_gy = a.frc_hx = a.frc_hy = a.les_tau = a.les_tau2 = a.les_c = T(0);
}
// (the seven slots that more than one model uses, as they stand: what lbm_debug_collision_args shows behind a model's values)
template <typename T> inline std::array<T, 7> shared_collision_slots(const KArgs<T>& a) {
    return {a.frc_gx, a.frc_gy, a.frc_hx, a.frc_hy, a.les_tau, a.les_tau2, a.les_c};
}
template <typename T> __host__ __device__ __forceinline__ BgkK<T> bgk_k(const KArgs<T>& a) { return {a.tau_inv}; }
template <typename T> inline void put(KArgs<T>& a, const BgkK<T>& k) { a.tau_inv = k.wp; }

template <typename T> __host__ __device__ __forceinline__ LesK<T> les_k(const KArgs<T>& a) { return {a.les_tau, a.les_tau2, a.les_c}; }
template <typename T> inline void put(KArgs<T>& a, const LesK<T>& k) { a.les_tau = k.tau; a.les_tau2 = k.tau2; a.les_c = k.c; }

template <typename T> __host__ __device__ __forceinline__ TrtK<T> trt_k(const KArgs<T>& a) { return {a.tau_inv, a.trt_wm, a.trt_wa, a.trt_wb}; }
template <typename T> inline void put(KArgs<T>& a, const TrtK<T>& k) { a.tau_inv = k.wp; a.trt_wm = k.wm; a.trt_wa = k.wa; a.trt_wb = k.wb; }

// (four values where the unions have three: the forced model's slots are the block in front of KArgs)
template <typename T> __host__ __device__ __forceinline__ ForcedK<T> forced_k(const KArgs<T>& a) { return {a.tau_inv, a.frc_gx, a.frc_gy, a.frc_hx, a.frc_hy}; }
template <typename T> inline void put(KArgs<T>& a, const ForcedK<T>& k) { a.tau_inv = k.wp; a.frc_gx = k.gx; a.frc_gy = k.gy; a.frc_hx = k.hx; a.frc_hy = k.hy; }

// (MRT is never TRT or forced as well: TRT's slots, and sb, kb in the first two of the forced model's, so that no field moves or is added)
template <typename T> __host__ __device__ __forceinline__ MrtK<T> mrt_k(const KArgs<T>& a) { return {a.tau_inv, a.trt_wm, a.trt_wa, a.trt_wb, a.frc_gx, a.frc_gy}; }
template <typename T> inline void put(KArgs<T>& a, const MrtK<T>& k) {
    a.tau_inv = k.wp; a.trt_wm = k.wm; a.trt_wa = k.wa; a.trt_wb = k.wb; a.frc_gx = k.sb; a.frc_gy = k.kb;
}

// the values of the model of an Arith value (the outlet sponge: none)
struct SpongeK {};
template <int AR, typename T>
__host__ __device__ __forceinline__ auto model_k(const KArgs<T>& a) {
    if constexpr (ar_mrt(AR)) return mrt_k(a);
    else if constexpr (ar_forced(AR)) return forced_k(a);
    else if constexpr (ar_trt(AR)) return trt_k(a);
    else if constexpr (ar_les(AR)) return les_k(a);
    else if constexpr (ar_sponge(AR)) return SpongeK{};
    else return bgk_k(a);
}

// The rate of column x on a sponge context (the sponge modes only; every other mode gets a zero that nothing reads). The index is
// clamped into the table: the lanes and region cells that have no column (x < 0, x >= nx: a region's overhang, a ragged nx, nx < 64)
// compute on zeros or garbage that is never stored, with the rate of the nearest column, and read nothing outside [0, nx).
template <typename T, int AR>
__device__ __forceinline__ T column_rate(const KArgs<T>& a, int x) {
    if constexpr (ar_sponge(AR)) return a.wp_x[x < 0 ? 0 : (x < a.nx ? x : a.nx - 1)];
    else return T(0);
}

// ---- strict operators: collision_step for one cell, LBMSolver.h:101-123, operation by operation ---------------------------------------
// rho and the momentum (moments i = 0..8 ascending from 0, N7); the caller divides with strict_div2 (a forced context adds h first).
// (The three sums are locals, returned: summed through references the chains come out interleaved, in other registers.)
template <typename T> struct Moments { T rho, jx, jy; };
template <typename T>
__device__ __forceinline__ Moments<T> strict_moments(const T (&f)[Q]) {
    T rho = T(0), jx = T(0), jy = T(0);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        rho += f[i];
        if (cx(i) != 0) jx += T(cx(i)) * f[i];
        if (cy(i) != 0) jy += T(cy(i)) * f[i];
    }
    return {rho, jx, jy};
}

// feq_i = w_i*rho*(1.0 + 3.0*cu + 4.5*cu*cu - 1.5*usq), cu = c_ix*ux + c_iy*uy with integer c (LBMSolver.h:119-121), evaluated
// operation by operation in the reference's order: ((1.0 + 3.0*cu) + (4.5*cu)*cu) - 1.5*usq. Shared WITHOUT changing a bit:
//  * where a component of c_i is 0 its product is an exact signed zero and the sum equals the other term bit for bit, except
//    for the sign of a zero result — which the bracket erases (1 + 3*(+-0) = 1, 4.5*(+-0)^2 = +0);
//  * opposite directions have cu of equal magnitude and opposite sign EXACTLY (negation is exact and rounding is symmetric:
//    (-1)*ux + (-1)*uy == -(ux + uy)), hence 3.0*cu flips its sign exactly and (4.5*cu)*cu is the same number: one cu, one
//    3*cu and one 4.5*cu*cu per PAIR, and 1.0 + (-t) is the subtraction 1.0 - t;
//  * 1.5*usq and the three w*rho are common to all directions.
// 112 instead of ~137 fp64 operations per cell (round 4); the populations stay np.array_equal to the oracle in every test.
// StrictEq: what is common to all directions. A pair's c.u: c1 = (1,0), c3 = (-1,0): ux; c2 = (0,1), c4 = (0,-1): uy;
// c5 = (1,1), c7 = (-1,-1): ux + uy; c8 = (1,-1), c6 = (-1,1): ux - uy (1*ux + (-1)*uy == ux - uy).
template <typename T> struct StrictEq { T c15, wr0, wr1, wr5; };
template <typename T>
__device__ __forceinline__ StrictEq<T> strict_eq(T rho, T ux, T uy) {
    const T usq = ux * ux + uy * uy;
    return {T(1.5) * usq, wgt<T>(0) * rho, wgt<T>(1) * rho, wgt<T>(5) * rho};
}
template <typename T>
__device__ __forceinline__ void strict_relax(T& fi, T wr, T bracket, T rate) {
    const T feq = wr * bracket;
    fi = fi - rate * (fi - feq);
}
template <typename T>
__device__ __forceinline__ void strict_relax_rest(T (&f)[Q], const StrictEq<T>& e, T rate) {
    strict_relax(f[0], e.wr0, (T(1.0) + T(0.0)) - e.c15, rate);      // cu = 0: 1.0 + 3.0*0 + 4.5*0*0 = 1.0 exactly
}

// BGK: every population relaxes with `rate`: the global wp, the cell's (LES) or the column's (sponge)
template <typename T>
__device__ __forceinline__ void strict_bgk(T (&f)[Q], const StrictEq<T>& e, T ux, T uy, T rate) {
    strict_relax_rest(f, e, rate);
    auto pair = [&](int i, int ib, T cu, T wr) {     // i: the direction whose c.u is `cu`; ib: its opposite
        const T t3 = T(3.0) * cu, t45 = (T(4.5) * cu) * cu;
        strict_relax(f[i], wr, ((T(1.0) + t3) + t45) - e.c15, rate);
        strict_relax(f[ib], wr, ((T(1.0) - t3) + t45) - e.c15, rate);
    };
    pair(1, 3, ux, e.wr1);
    pair(2, 4, uy, e.wr1);
    pair(5, 7, ux + uy, e.wr5);
    pair(8, 6, ux - uy, e.wr5);
}

// Smagorinsky relaxation rate of one cell, 1/tau_eff with tau_eff = (tau + sqrt(tau^2 + C*|Pi_neq|/rho))/2: the closed form of
// tau = tau0 + 3 Cs^2 |S|, |S| = sqrt(2 S:S), for cs^2 = 1/3 and dx = dt = 1, where Pi_neq is the non-equilibrium momentum flux of
// the post-BC populations. STRICT: the operation tree of the issue's reference operator (tests/test_gpu_les.py les_collide) in IEEE
// arithmetic with correctly rounded square roots and divisions, on ux, uy already divided by rho — bit-identical to numpy.
template <typename T>
__device__ __forceinline__ T les_tau_inv_strict(const T (&f)[Q], T rho, T ux, T uy, const LesK<T>& k) {
    const T sxx = ((((f[1] + f[3]) + f[5]) + f[6]) + f[7]) + f[8];
    const T syy = ((((f[2] + f[4]) + f[5]) + f[6]) + f[7]) + f[8];
    const T sxy = ((f[5] - f[6]) + f[7]) - f[8];
    const T pxx = (sxx - rho * (ux * ux)) - rho * T(1.0 / 3.0);
    const T pyy = (syy - rho * (uy * uy)) - rho * T(1.0 / 3.0);
    const T pxy = sxy - rho * (ux * uy);
    const T qn = sqrt_t((pxx * pxx + pyy * pyy) + T(2.0) * (pxy * pxy));
    const T tau_eff = T(0.5) * (k.tau + sqrt_t(k.tau2 + k.c * (qn / rho)));
    return T(1.0) / tau_eff;
}

// the two feq of a pair, then the even (np) and odd (nm) non-equilibrium parts of the pair: what TRT and MRT relax
template <typename T>
__device__ __forceinline__ void strict_pair_parts(const T (&f)[Q], const StrictEq<T>& e, int i, int ib, T cu, T wr, T& np, T& nm) {
    const T t3 = T(3.0) * cu, t45 = (T(4.5) * cu) * cu;
    const T feq = wr * (((T(1.0) + t3) + t45) - e.c15), feqb = wr * (((T(1.0) - t3) + t45) - e.c15);
    np = T(0.5) * ((f[i] + f[ib]) - (feq + feqb));
    nm = T(0.5) * ((f[i] - f[ib]) - (feq - feqb));
}

// TRT (tests/test_gpu_trt.py trt_collide, operation by operation): the parts of each pair, relaxed with wp = 1/tau and wm = 1/tau_minus;
// the rest population with wp
template <typename T>
__device__ __forceinline__ void strict_trt(T (&f)[Q], const StrictEq<T>& e, T ux, T uy, const TrtK<T>& k) {
    strict_relax_rest(f, e, k.wp);
    auto pair = [&](int i, int ib, T cu, T wr) {
        T np, nm;
        strict_pair_parts(f, e, i, ib, cu, wr, np, nm);
        const T wpn = k.wp * np, wmn = k.wm * nm;
        f[i] = (f[i] - wpn) - wmn;
        f[ib] = (f[ib] - wpn) + wmn;
    };
    pair(1, 3, ux, e.wr1);
    pair(2, 4, uy, e.wr1);
    pair(5, 7, ux + uy, e.wr5);
    pair(8, 6, ux - uy, e.wr5);
}

// MRT (tests/mrt_reference.py mrt_collide, operation by operation): TRT's np, nm of each pair; the first pair (1,3 / 5,7) of a group
// leaves them, the second (2,4 / 8,6; `jj`, `jb`: the first pair's directions) forms the group's half sum and half difference of the
// even parts, relaxes the half sum with the bulk rate sb and the half difference with wp, and finishes all four populations. The rest
// population relaxes with the bulk rate.
template <typename T>
__device__ __forceinline__ void strict_mrt(T (&f)[Q], const StrictEq<T>& e, T ux, T uy, const MrtK<T>& k) {
    strict_relax_rest(f, e, k.sb);
    T np1 = T(0), wmn1 = T(0);      // the even part and the relaxed odd part of a group's first pair, kept for its second
    auto first = [&](int i, int ib, T cu, T wr) {
        T nm;
        strict_pair_parts(f, e, i, ib, cu, wr, np1, nm);
        wmn1 = k.wm * nm;
    };
    auto second = [&](int i, int ib, int jj, int jb, T cu, T wr) {
        T np, nm;
        strict_pair_parts(f, e, i, ib, cu, wr, np, nm);
        const T wmn = k.wm * nm;
        const T tr = T(0.5) * (np1 + np), dv = T(0.5) * (np1 - np);
        const T st = k.sb * tr, wd = k.wp * dv;
        const T ep = st + wd, eq = st - wd;
        f[jj] = (f[jj] - ep) - wmn1;
        f[jb] = (f[jb] - ep) + wmn1;
        f[i] = (f[i] - eq) - wmn;
        f[ib] = (f[ib] - eq) + wmn;
    };
    first(1, 3, ux, e.wr1);
    second(2, 4, 1, 3, uy, e.wr1);
    first(5, 7, ux + uy, e.wr5);
    second(8, 6, 5, 7, ux - uy, e.wr5);
}

// Guo's source (tests/forcing_reference.py guo_collide, operation by operation), added to BGK's relaxed populations:
//     S_i = w_i * ((3 cg - u3) + (9 cu) cg),  u3 = 3 (ux gx + uy gy),  cg = c_i.g; the opposite direction negates 3 cg and keeps the product.
// A phase of its own behind an empty asm statement, as in the contracted arithmetic: what the relaxation held is dead by now.
template <typename T>
__device__ __forceinline__ void strict_guo(T (&f)[Q], T ux, T uy, T gx, T gy) {
    asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]), "+v"(f[8]), "+v"(ux), "+v"(uy));
    const T u3 = T(3.0) * (ux * gx + uy * gy);
    f[0] = f[0] + wgt<T>(0) * (T(0.0) - u3);
    auto source = [&](int i, int ib, T cu, T cg, T w) {
        const T sa = T(3.0) * cg, sb = (T(9.0) * cu) * cg;
        f[i] = f[i] + w * ((sa - u3) + sb);
        f[ib] = f[ib] + w * (((-sa) - u3) + sb);
    };
    source(1, 3, ux, gx, wgt<T>(1));
    source(2, 4, uy, gy, wgt<T>(1));
    source(5, 7, ux + uy, gx + gy, wgt<T>(5));
    source(8, 6, ux - uy, gx - gy, wgt<T>(5));
}

// ---- contracted operators --------------------------------------------------------------------------------------------------------------
// moments as short trees over opposite pairs (depth 4 / 3 instead of chains of 9 / 6 dependent additions); the pair sums stay at hand
// for the operators that take sums of populations (LES, MRT). jx, jy: the momentum rho u (a forced context adds h to it); sa, sd: the
// sums of the axis and of the diagonal populations, which fp64 MRT takes (formed here, while the pair sums are at hand: formed later they
// cost the fp64 register kernel five spilled VGPRs; dead in every other kernel)
template <typename T> struct PairMoments { T a13, a24, a57, a68, rho, jx, jy, sa, sd; };
template <typename T>
__device__ __forceinline__ PairMoments<T> pair_moments(const T (&f)[Q]) {
    PairMoments<T> m;
    m.a13 = f[1] + f[3]; m.a24 = f[2] + f[4]; m.a57 = f[5] + f[7]; m.a68 = f[6] + f[8];
    const T d13 = f[1] - f[3], d24 = f[2] - f[4], d57 = f[5] - f[7], d68 = f[6] - f[8];
    m.rho = ((f[0] + m.a13) + (m.a24 + m.a57)) + m.a68;
    m.jx = (d13 + d57) - d68;
    m.jy = (d24 + d57) + d68;
    m.sa = m.a13 + m.a24; m.sd = m.a57 + m.a68;
    return m;
}
// v = 3u. 1 + 3cu + 4.5cu^2 - 1.5u^2 = base + cv*(1 + 0.5cv) with cv = c.v and base = 1 - v^2/6: the inner bracket
// is one FMA with INLINE constants (0.5, 1.0). gfx950 VALU instructions take one SGPR/literal operand at most, so
// fma(4.5, cu, 3.0) cost two v_mov per direction to build the 3.0 — 16 of ~100 vector instructions per cell.
// In two steps, the velocity and what the equilibrium shares, because the LES rate is formed between them (from 1/rho; behind the second
// step its kernels come out with other instructions).
template <typename T> struct ContractedEq { T rinv, inv3, vx, vy, base, wr0, wr1, wr5; };
template <typename T>
__device__ __forceinline__ void contracted_velocity(const PairMoments<T>& m, ContractedEq<T>& e) {
    e.rinv = recip_t(m.rho);
    e.inv3 = e.rinv * T(3.0);
    e.vx = m.jx * e.inv3; e.vy = m.jy * e.inv3;
}
template <typename T>
__device__ __forceinline__ void contracted_eq(const PairMoments<T>& m, ContractedEq<T>& e) {
    e.base = fma_t(T(-1.0 / 6.0), fma_t(e.vx, e.vx, e.vy * e.vy), T(1.0));
    e.wr0 = wgt<T>(0) * m.rho; e.wr1 = wgt<T>(1) * m.rho; e.wr5 = wgt<T>(5) * m.rho;
}

// BGK: every population relaxes with `rate`: the global wp, the cell's (LES) or the column's (sponge).
// The three w rho are formed here, beside the loop that selects among them, not taken from `e` (where they are then dead): the compiler
// folds the selection into the products before it unrolls, and with the products out of its sight the BGK kernels come out in another
// instruction order.
template <typename T>
__device__ __forceinline__ void contracted_bgk(T (&f)[Q], const ContractedEq<T>& e, T rho, T rate) {
    const T wr0 = wgt<T>(0) * rho, wr1 = wgt<T>(1) * rho, wr5 = wgt<T>(5) * rho;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        T cv;
        if (cx(i) == 0 && cy(i) == 0) cv = T(0);
        else if (cy(i) == 0) cv = T(cx(i)) * e.vx;
        else if (cx(i) == 0) cv = T(cy(i)) * e.vy;
        else cv = T(cx(i)) * e.vx + T(cy(i)) * e.vy;
        const T t = (i == 0) ? e.base : fma_t(cv, fma_t(cv, T(0.5), T(1.0)), e.base);
        const T wr = i == 0 ? wr0 : (i < 5 ? wr1 : wr5);
        f[i] = fma_t(rate, fma_t(wr, t, -f[i]), f[i]);     // f - (f - feq)/tau = f + (feq - f)/tau
    }
}

// the Smagorinsky rate (les_tau_inv_strict) with FMAs on the momenta: Pi_neq = S - j j / rho - rho/3 I
template <typename T>
__device__ __forceinline__ T les_tau_inv_contracted(const PairMoments<T>& m, T rinv, const LesK<T>& k) {
    const T sxx = (m.a13 + m.a57) + m.a68, syy = (m.a24 + m.a57) + m.a68, sxy = m.a57 - m.a68;
    const T jxr = m.jx * rinv;
    const T third = m.rho * T(-1.0 / 3.0);
    const T pxx = fma_t(-jxr, m.jx, sxx + third), pyy = fma_t(-m.jy * rinv, m.jy, syy + third), pxy = fma_t(-jxr, m.jy, sxy);
    const T qn = sqrt_c(fma_t(pxx, pxx, fma_t(pyy, pyy, T(2.0) * (pxy * pxy))));
    return T(2.0) * recip_t(k.tau + sqrt_c(fma_t(k.c, qn * rinv, k.tau2)));
}

template <typename T>
__device__ __forceinline__ void contracted_relax_rest(T (&f)[Q], const ContractedEq<T>& e, T rate) {
    f[0] = fma_t(rate, fma_t(e.wr0, e.base, -f[0]), f[0]);
}
// One pair of TRT's and MRT's: f_i' = f_i + wa (feq_i - f_i) + wb (feq_ib - f_ib) with wa = (wp + wm)/2, wb = (wp - wm)/2: BGK's residuals
// of the two directions (c.v changes its sign for the opposite one), then two FMAs each, in place. Two temporaries beyond BGK's.
// i: the direction whose c.v is `cv`; ib: its opposite; b: the base. ADD_G (fp32 MRT): g joins the two populations behind their residuals.
template <bool ADD_G = false, typename T>
__device__ __forceinline__ void contracted_pair(T (&f)[Q], int i, int ib, T cv, T wr, T b, T wa, T wb, T g = T(0)) {
    const T ri = fma_t(wr, fma_t(cv, fma_t(cv, T(0.5), T(1.0)), b), -f[i]);
    const T rb = fma_t(wr, fma_t(cv, fma_t(cv, T(0.5), T(-1.0)), b), -f[ib]);
    if constexpr (ADD_G) { f[i] += g; f[ib] += g; }
    f[i] = fma_t(wa, ri, fma_t(wb, rb, f[i]));
    f[ib] = fma_t(wa, rb, fma_t(wb, ri, f[ib]));
}
// One pair after the other: an empty asm statement that "rewrites" a finished pair together with the next pair's inputs keeps
// the compiler from starting the next pair's residuals early (it would hold all eight and spill in the fp64 register kernel).
template <typename T>
__device__ __forceinline__ void pair_then(T (&f)[Q], int i, int ib, int j, int jb) {
    asm volatile("" : "+v"(f[i]), "+v"(f[ib]), "+v"(f[j]), "+v"(f[jb]));
}
// The four pairs of TRT (bd = ba = base) and of fp64 MRT (the diagonal pairs on the base bd, the axis pairs on ba)
template <typename T>
__device__ __forceinline__ void contracted_pairs(T (&f)[Q], const ContractedEq<T>& e, T wa, T wb, T bd, T ba) {
    contracted_pair(f, 5, 7, e.vx + e.vy, e.wr5, bd, wa, wb);
    pair_then(f, 5, 7, 8, 6);
    contracted_pair(f, 8, 6, e.vx - e.vy, e.wr5, bd, wa, wb);
    pair_then(f, 8, 6, 1, 3);
    contracted_pair(f, 1, 3, e.vx, e.wr1, ba, wa, wb);
    pair_then(f, 1, 3, 2, 4);
    contracted_pair(f, 2, 4, e.vy, e.wr1, ba, wa, wb);
}

// MRT is TRT plus the same g = (sb - wp)/4 S on the four populations of a group (the axis pairs; the diagonal pairs), S the sum
// of the group's four residuals (-4 ta, -4 td), with the rest population relaxed by sb. Since wa + wb = wp, raising the
// equilibrium's `base` of a group by g / (wp w rho) adds exactly g to each of its populations: a group runs TRT's pair code
// on a base of its own, and nothing but that base is alive beyond TRT's values. With t = 1 - base = |v|^2 / 6, 4 w5 = w1 and
// kb = (sb - wp) / (4 wp) folded on the host:  base_axes = base + kb ((4 + 2 t) - 9 (f1 + f2 + f3 + f4) / rho),
// base_diagonals = base + 4 kb ((1 + 2 t) - 9 (f5 + f6 + f7 + f8) / rho), in inline constants only (a VALU instruction reads
// one scalar register or literal at most). That is the fp64 form; fp32 adds g itself (contracted_mrt_f32).
template <typename T>
__device__ __forceinline__ void contracted_mrt(T (&f)[Q], const PairMoments<T>& m, const ContractedEq<T>& e, const MrtK<T>& k) {
    contracted_relax_rest(f, e, k.sb);
    const T t2 = T(2.0) * (T(1.0) - e.base);
    auto nine_over_rho = [&](T sum) { const T x = sum * e.inv3; return fma_t(T(2.0), x, x); };
    T ba = fma_t(k.kb, (t2 + T(4.0)) - nine_over_rho(m.sa), e.base);
    T bd = fma_t(k.kb, T(4.0) * ((t2 + T(1.0)) - nine_over_rho(m.sd)), e.base);
    asm volatile("" : "+v"(ba), "+v"(bd));
    contracted_pairs(f, e, k.wa, k.wb, bd, ba);
}
// fp32: the shift of the base costs the register kernel a wave of occupancy (84 to 86 VGPRs where 80 are the limit); g
// itself, formed in front of its group from the populations the group is about to replace and added to them, does not
template <typename T>
__device__ __forceinline__ void contracted_mrt_f32(T (&f)[Q], const ContractedEq<T>& e, const MrtK<T>& k) {
    contracted_relax_rest(f, e, k.sb);
    auto group = [&](int i, int ib, int j, int jb, T n) {
        const T sum = ((f[i] + f[ib]) + f[j]) + f[jb];
        return k.kb * (k.wp * fma_t(e.wr1, fma_t(T(2.0), T(1.0) - e.base, n), -sum));
    };
    T g = group(5, 7, 8, 6, T(1.0));
    contracted_pair<true>(f, 5, 7, e.vx + e.vy, e.wr5, e.base, k.wa, k.wb, g);
    pair_then(f, 5, 7, 8, 6);
    contracted_pair<true>(f, 8, 6, e.vx - e.vy, e.wr5, e.base, k.wa, k.wb, g);
    pair_then(f, 8, 6, 1, 3);
    g = group(1, 3, 2, 4, T(4.0));
    contracted_pair<true>(f, 1, 3, e.vx, e.wr1, e.base, k.wa, k.wb, g);
    pair_then(f, 1, 3, 2, 4);
    contracted_pair<true>(f, 2, 4, e.vy, e.wr1, e.base, k.wa, k.wb, g);
}

// Guo's source, added once BGK's chain has finished. With cg = c_i.g and cv = c_i.v:
//     S_i = w_i (3 cg - 3 u.g + 9 (c_i.u) cg) = 3 w_i ((cg cv - u.g) + cg),   the opposite direction 3 w_i ((cg cv - u.g) - cg)
// so a pair shares m = cg cv - u.g, and gx, gy enter as scalar operands only (no uniform value is formed in a vector register).
// A phase of its own behind an empty asm statement that "rewrites" its inputs: base and the three w rho are dead by now and
// u.g is not yet alive, so the kernel holds no more values at once than BGK's does (folded into the relaxation, the
// register kernels of fp64 spilled: profiles/forcing/README.md).
template <typename T>
__device__ __forceinline__ void contracted_guo(T (&f)[Q], T vx, T vy, T gx, T gy) {
    T sx = vx, sy = vy;
    asm volatile("" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]), "+v"(f[8]), "+v"(sx), "+v"(sy));
    const T ug = fma_t(sx, gx, sy * gy) * T(1.0 / 3.0);      // u.g
    f[0] = fma_t(T(-4.0 / 3.0), ug, f[0]);                  // S_0 = -3 w_0 u.g
    auto source = [&](int i, int ib, T w3, T mi, T mb) {     // mi = m + cg, mb = m - cg; w3 = 3 w_i
        f[i] = fma_t(w3, mi, f[i]);
        f[ib] = fma_t(w3, mb, f[ib]);
    };
    {   const T m = fma_t(gx, sx, -ug); source(1, 3, T(1.0 / 3.0), m + gx, m - gx); }
    {   const T m = fma_t(gy, sy, -ug); source(2, 4, T(1.0 / 3.0), m + gy, m - gy); }
    {   const T cv = sx + sy, m = fma_t(gx, cv, fma_t(gy, cv, -ug)); source(5, 7, T(1.0 / 12.0), (m + gx) + gy, (m - gx) - gy); }
    {   const T cv = sx - sy, m = fma_t(gx, cv, fma_t(-gy, cv, -ug)); source(8, 6, T(1.0 / 12.0), (m + gx) - gy, (m - gx) + gy); }
}

// ---- the collision of the step kernels: the one place that picks operators by Arith ---------------------------------------------------
// `wpx`: column_rate of the cell's column (read by the sponge modes only)
template <typename T, int AR>
__device__ __forceinline__ void collide(T (&f)[Q], const KArgs<T>& a, T wpx) {
    static_assert(!(ar_les(AR) && ar_trt(AR)), "TRT and LES exclude each other");
    static_assert(!(ar_forced(AR) && (ar_les(AR) || ar_trt(AR))), "forcing excludes LES and TRT");
    static_assert(!(ar_mrt(AR) && (ar_les(AR) || ar_trt(AR) || ar_forced(AR))), "MRT excludes LES, TRT and forcing");
    static_assert(!(ar_sponge(AR) && (AR & 30) != 0), "the sponge excludes LES, TRT, forcing and MRT");
    // the model's values, read before anything is computed (where the kernels have always loaded them)
    [[maybe_unused]] const auto k = model_k<AR>(a);
    if constexpr (ar_contracted(AR)) {
        PairMoments<T> m = pair_moments(f);
        if constexpr (ar_forced(AR)) { m.jx = m.jx + k.hx; m.jy = m.jy + k.hy; }      // Guo: the momenta take h = F/2, so v is 3u of the forced velocity
        ContractedEq<T> e;
        contracted_velocity(m, e);
        T les_rate = T(0);
        if constexpr (ar_les(AR)) les_rate = les_tau_inv_contracted(m, e.rinv, k);
        contracted_eq(m, e);
        if constexpr (ar_mrt(AR)) {
            if constexpr (sizeof(T) == 4) contracted_mrt_f32(f, e, k);
            else contracted_mrt(f, m, e, k);
        } else if constexpr (ar_trt(AR)) {
            contracted_relax_rest(f, e, k.wp);
            contracted_pairs(f, e, k.wa, k.wb, e.base, e.base);
        } else if constexpr (ar_forced(AR)) {
            contracted_bgk(f, e, m.rho, k.wp);
            contracted_guo(f, e.vx, e.vy, k.gx, k.gy);
        } else if constexpr (ar_les(AR)) contracted_bgk(f, e, m.rho, les_rate);
        else if constexpr (ar_sponge(AR)) contracted_bgk(f, e, m.rho, wpx);
        else contracted_bgk(f, e, m.rho, k.wp);
    } else {
        const Moments<T> m = strict_moments(f);
        T rho = m.rho, ux = m.jx, uy = m.jy;
        if constexpr (ar_forced(AR)) { ux = ux + k.hx; uy = uy + k.hy; }      // Guo: the momenta take h = F/2 before the divisions
        strict_div2(ux, uy, rho);
        T les_rate = T(0);
        if constexpr (ar_les(AR)) les_rate = les_tau_inv_strict(f, rho, ux, uy, k);
        const StrictEq<T> e = strict_eq(rho, ux, uy);
        if constexpr (ar_mrt(AR)) strict_mrt(f, e, ux, uy, k);
        else if constexpr (ar_trt(AR)) strict_trt(f, e, ux, uy, k);
        else if constexpr (ar_forced(AR)) {
            strict_bgk(f, e, ux, uy, k.wp);
            strict_guo(f, ux, uy, k.gx, k.gy);
        } else if constexpr (ar_les(AR)) strict_bgk(f, e, ux, uy, les_rate);
        else if constexpr (ar_sponge(AR)) strict_bgk(f, e, ux, uy, wpx);
        else strict_bgk(f, e, ux, uy, k.wp);
    }
}

}  // namespace lbmk
