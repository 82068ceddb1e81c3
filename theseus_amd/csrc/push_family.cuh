// What the planar-pushing forward (push_kernels.hip: thx_push2_eval, thx_push2_error) and its implicit backward
// (push_vjp_kernels.hip: thx_push2_vjp) share: the pose and aux loads, the SE2 pieces both evaluate and the guards that decide
// which terms are skipped.  Included after the source's own ``#pragma clang fp contract(off)``.
#pragma once
#include "term_family.cuh"
#include "lie_se2.cuh"

namespace thx {

// one pose record as ONE vector load (the record is 4 * sizeof(T) aligned: checked on the host)
__device__ __forceinline__ SE2<float> load_pose(const float* __restrict__ x, int64_t rec) {
  const float4 v = reinterpret_cast<const float4*>(x)[rec];
  return SE2<float>{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ SE2<double> load_pose(const double* __restrict__ x, int64_t rec) {
  const double4 v = reinterpret_cast<const double4*>(x)[rec];
  return SE2<double>{v.x, v.y, v.z, v.w};
}

template <typename T>
__device__ __forceinline__ SE2<T> aux_pose(const thx_push2_term& tm, int k, int b) {
  const T* p = static_cast<const T*>(tm.aux[k]) + (int64_t)b * tm.aux_bstride[k];
  return SE2<T>{p[0], p[1], p[2], p[3]};
}

// the 1 | 3 row weights of a Scale / DiagonalCostWeight at aux slot k
template <typename T>
__device__ __forceinline__ void row_weights(const thx_push2_term& tm, int k, int b, T* w) {
  w[0] = aux_at<T>(tm, k, b, 0);
  w[1] = tm.wdim == 3 ? aux_at<T>(tm, k, b, 1) : w[0];
  w[2] = tm.wdim == 3 ? aux_at<T>(tm, k, b, 2) : w[0];
}

// R^T p (so2.py: unrotate = rotate with (cos, -sin))
template <typename T>
__device__ __forceinline__ void unrotate(T c, T s, T px, T py, T& rx, T& ry) {
  const T ns = -s;
  rx = c * px - ns * py;
  ry = ns * px + c * py;
}

// between with the reference's Jacobian of the first argument: Ad(B^-1) (-Ad(A))  (lie_group.py:125-136,162-178); the second is I
template <typename T>
__device__ __forceinline__ void between_j0(const SE2<T>& A, const SE2<T>& B, SE2<T>& D, T* J0, bool want_jac) {
  SE2<T> Ai, Bi;
  se2_inv(A, Ai);
  se2_mul(Ai, B, D);
  if (!want_jac) return;
  se2_inv(B, Bi);
  T AdB[9], AdA[9];
  se2_adjoint(Bi, AdB);
  se2_adjoint(A, AdA);
#pragma unroll
  for (int i = 0; i < 9; ++i) AdA[i] = -AdA[i];
  mat3_mul(AdB, AdA, J0);
}

__device__ __forceinline__ int push_dim(int kind) { return kind == THX_PUSH2_CONTACT ? 1 : 3; }
__device__ __forceinline__ int push_vars(int kind) { return kind == THX_PUSH2_CONTACT ? 2 : (kind == THX_PUSH2_PRIOR ? 1 : 4); }

// the kind is one of the four, every pose a term reads lies inside the state, its weight width is 1 or 3
__device__ __forceinline__ bool push_reads_ok(const thx_push2_term& tm, int V) {
  if (tm.kind < THX_PUSH2_QSP || tm.kind > THX_PUSH2_PRIOR) return false;
  const int nv = push_vars(tm.kind);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < nv && (tm.pose[s] < 0 || tm.pose[s] >= V)) return false;
  if (tm.kind == THX_PUSH2_CONTACT) return tm.rows >= 1 && tm.cols >= 1;
  return tm.wdim == 1 || tm.wdim == 3;
}

// ... and its rows and blocks lie inside e (m rows) and J (j_total elements per problem)
__device__ __forceinline__ bool push_writes_ok(const thx_push2_term& tm, int m, int64_t j_total) {
  const int dim = push_dim(tm.kind), nv = push_vars(tm.kind);
  return !(tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)3 * dim * nv > j_total);
}

template <typename T>
inline Eps2<T> make_eps2(const thx_se2_eps* e) {
  return Eps2<T>{(T)e->near_zero, (T)e->d_near_zero};
}

}  // namespace thx
