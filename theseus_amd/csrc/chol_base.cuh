#pragma once
#include "common.cuh"

#include <type_traits>
#include <utility>

namespace thx {

constexpr int TILE = THX_TILE;

// compile-time loop: the body sees the index as a constant expression, so every register-array
// subscript below is static (a plain `#pragma unroll` over 128 fat iterations is refused by the
// optimiser and would push the row registers to scratch)
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;

template <typename T>
struct CT;
template <>
struct CT<float> {
  static constexpr int KB = 32, LDT = 36, VEC = 4, LDM = 132, LDB = 36;
  using V = float4;
};
template <>
struct CT<double> {
  // k-chunks of 16 columns, two of them in flight (kloop_f: AHEAD).  32-column chunks -- KB = 32, LDT = 34: everything below is
  // written for either -- halve the barriers and staging round trips per flop and measured SLOWER: factor 111.2 vs 108.8 ms at
  // n = 1536 / batch 4096, 27.8 vs 26.3 ms at batch 1024, 44.7 vs 43.6 ms at n = 3072 / batch 256 on one box
  // (profiles/r3/j_ab_f64_kchunk32_vs_16.txt): the fp64 K-loop is not barrier-bound; with 70 KB of staging per workgroup the two
  // workgroups of a CU leave no LDS slack and one 32-column chunk in flight hides less latency than two 16-column ones.
  static constexpr int KB = 16, LDT = 18, VEC = 2, LDM = 130, LDB = 34;
  using V = double2;
};

// The diagonal tile in LDS (chol_diag): only its ten lower 32x32 sub-blocks, each stored row-major with row stride LDB
// (= 4 banks mod 32, like the 128-wide rows they replace: 46 KB instead of 68 KB in fp32 -> three workgroups per CU).
template <typename T>
__device__ __forceinline__ constexpr int tblk(int u, int v) {
  return (u * (u + 1) / 2 + v) * 32 * CT<T>::LDB;
}

// 1/sqrt(d) from the hardware estimate + Newton steps (~1 ulp): the pivot scaling of the in-register
// Cholesky sits on a 128-step latency chain, a correctly rounded sqrt + division is ~40 dependent
// instructions, this is ~8.  L[c][c] = d * isq and L[r][c] = S[r][c] * isq stay mutually consistent.
__device__ __forceinline__ float t_rsqrt(float d) {
  float y = __builtin_amdgcn_rsqf(d);
  return y * (1.5f - 0.5f * d * y * y);
}
__device__ __forceinline__ double t_rsqrt(double d) {
  double y = __builtin_amdgcn_rsq(d);
  y = y * (1.5 - 0.5 * d * y * y);
  return y * (1.5 - 0.5 * d * y * y);
}

// lane broadcast through SGPRs (v_readlane_b32; `l` is wave uniform)
__device__ __forceinline__ float bcast(float x, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}
__device__ __forceinline__ double bcast(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                          __builtin_amdgcn_readlane(__double2loint(x), l));
}

}  // namespace thx
