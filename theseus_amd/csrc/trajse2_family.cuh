// What the SE2 motion planner's forward (trajse2_kernels.hip: thx_trajse2_eval, thx_trajse2_error, thx_trajse2_retract) and its
// implicit backward (trajse2_vjp_kernels.hip: thx_trajse2_vjp) share: the record load, the row weights, the sizes of a kind and the
// guard that decides which terms are skipped.  Included after the source's own ``#pragma clang fp contract(off)``.
#pragma once
#include "term_family.cuh"
#include "lie_se2.cuh"

namespace thx {

// one state record as ONE vector load (the record is 4 * sizeof(T) aligned: checked on the host)
__device__ __forceinline__ SE2<float> tse2_load(const float* __restrict__ x, int64_t rec) {
  const float4 v = reinterpret_cast<const float4*>(x)[rec];
  return SE2<float>{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ SE2<double> tse2_load(const double* __restrict__ x, int64_t rec) {
  const double4 v = reinterpret_cast<const double4*>(x)[rec];
  return SE2<double>{v.x, v.y, v.z, v.w};
}

// the row weights of a Scale (wdim 1) / DiagonalCostWeight (wdim = n) at aux slot k
template <typename T, int n>
__device__ __forceinline__ void tse2_weights(const thx_trajse2_term& tm, int k, int b, T* w) {
  w[0] = aux_at<T>(tm, k, b, 0);
#pragma unroll
  for (int i = 1; i < n; ++i) w[i] = tm.wdim == n ? aux_at<T>(tm, k, b, i) : w[0];
}

__device__ __forceinline__ int tse2_dim(int kind) {
  return kind == THX_TRAJSE2_GP ? 6
         : (kind == THX_TRAJSE2_COLLISION || kind == THX_TRAJSE2_NONHOLONOMIC) ? 1
         : (kind == THX_TRAJSE2_PRIOR_XY ? 2 : 3);
}
__device__ __forceinline__ int tse2_vars(int kind) {
  return kind == THX_TRAJSE2_GP ? 4 : (kind == THX_TRAJSE2_NONHOLONOMIC ? 2 : 1);
}

// the kind is one of the seven, every record a term reads lies inside the state, a weight is as wide as 1 or as the cost
__device__ __forceinline__ bool tse2_reads_ok(const thx_trajse2_term& tm, int V) {
  if (tm.kind < THX_TRAJSE2_COLLISION || tm.kind > THX_TRAJSE2_PRIOR_XY) return false;
  const int nv = tse2_vars(tm.kind);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < nv && (tm.var[s] < 0 || tm.var[s] >= V)) return false;
  if (tm.kind == THX_TRAJSE2_COLLISION) return tm.rows >= 1 && tm.cols >= 1;
  if (tm.kind == THX_TRAJSE2_GP || tm.kind == THX_TRAJSE2_NONHOLONOMIC) return true;
  return tm.wdim == 1 || tm.wdim == tse2_dim(tm.kind);
}

template <typename T>
inline Eps2<T> tse2_eps(const thx_se2_eps* e) {
  return Eps2<T>{(T)e->near_zero, (T)e->d_near_zero};
}

}  // namespace thx
