// What the fused cost families (traj_kernels.hip, push_kernels.hip, trajse2_kernels.hip, homog_kernels.hip, kin_kernels.hip) share: a family evaluates a whole objective
// from a table of 128-byte terms (thx_traj2_term, thx_push2_term, thx_trajse2_term of include/theseus_hip.h: the same layout, the
// variable field named by the family).
// Here: the per-term aux accessor, the bilinear signed-distance lookup, the fixed-order reduction of a *_error kernel and the host
// checks of the exports.  The term functions, the two __global__ functions and the exports stay with the family.
#pragma once
#include "common.cuh"

namespace thx {

constexpr int kErrThreads = 256;   // workgroup of a *_error kernel

// element i of problem b's values of aux slot k (aux_bstride: the tensor's own batch stride, 0 for a shared one)
template <typename T, typename Term>
__device__ __forceinline__ T aux_at(const Term& tm, int k, int b, int i = 0) {
  return static_cast<const T*>(tm.aux[k])[(int64_t)b * tm.aux_bstride[k] + i];
}

// SignedDistanceField2D.signed_distance (signed_distance_field.py:163-241) at one point (px, py) of an R x C grid with origin
// (ox, oy): the bilinear value and its derivatives w.r.t. px, py; all three zero outside the grid (sdf_boundary_value = 0).  Runs in
// the run's dtype with contraction off and in the reference's operation order, so a kink lands where the torch classes put it.
template <typename T>
__device__ __forceinline__ void sdf_bilinear(const T* __restrict__ sdf, int R, int C, T ox, T oy, T cell, T px, T py, T& dist, T& j1,
                                             T& j2) {
#pragma clang fp contract(off)
  // signed_distance_field.py:179-187
  const bool oob = (px < ox) || (px > (ox + (T)(C - 1.0) * cell)) || (py < oy) || (py > (oy + (T)(R - 1.0) * cell));
  const T col = (px - ox) / cell, row = (py - oy) / cell;
  // :198-205 (the clamp is applied before the conversion: the same indices, and no out-of-range conversion)
  const T lr = floor(row), lc = floor(col), hr = lr + (T)1, hc = lc + (T)1;
  auto idx = [](T v, int hi) {
    if (!(v > (T)0)) return 0;   // (also NaN)
    return v < (T)hi ? (int)v : hi;
  };
  const int lri = idx(lr, R - 1), lci = idx(lc, C - 1), hri = idx(hr, R - 1), hci = idx(hc, C - 1);
  const T sll = sdf[(int64_t)lri * C + lci], shl = sdf[(int64_t)hri * C + lci];
  const T slh = sdf[(int64_t)lri * C + hci], shh = sdf[(int64_t)hri * C + hci];
  const T hrd = hr - row, hcd = hc - col, lrd = row - lr, lcd = col - lc;
  dist = hrd * hcd * sll + lrd * hcd * shl + hrd * lcd * slh + lrd * lcd * shh;   // :215-220
  j1 = (hrd * (slh - sll) + lrd * (shh - shl)) / cell;                             // :231-238
  j2 = (hcd * (shl - sll) + lcd * (shh - slh)) / cell;
  if (oob) dist = (T)0, j1 = (T)0, j2 = (T)0;
}

// err = 0.5 * (sum of the workgroup's kErrThreads fp64 partials), by a fixed-order tree: deterministic, no atomics
template <typename T>
__device__ __forceinline__ void store_half_sum(double acc, T* __restrict__ err) {
  __shared__ double part[kErrThreads];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kErrThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *err = (T)(0.5 * part[0]);
}

// What every export checks on the host before any launch.  ``any_null``: one of the family's pointers is null; ``bad_size``: the
// message of the family's own size check that fails (it comes after the batch, before the alignment), or nullptr; ``x_vec``: the
// elements of the state that one load reads.
inline int family_check(const char* who, bool any_null, const void* terms, int32_t n_terms, const void* x, int x_vec, int32_t B,
                        int dtype, const char* bad_size) {
  if (any_null || !terms || !x) return fail(who, ": null pointer");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (n_terms < 1) return fail(who, ": n_terms < 1");
  if (B < 1) return fail(who, ": empty batch");
  if (bad_size) return fail(who, bad_size);
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  if (reinterpret_cast<uintptr_t>(terms) % 8 || reinterpret_cast<uintptr_t>(x) % (x_vec * el)) return fail(who, ": pointer not aligned");
  return 0;
}

// ... and what an *_eval export checks after that; ``short_j``: the family's message for a j_total below one block row.
// -> the grid of one thread per (term, problem) in ``blocks``
inline int family_check_eval(const char* who, const void* J, const char* short_j, const void* e, int64_t lde, int32_t m,
                             int32_t n_terms, int32_t B, int dtype, unsigned* blocks) {
  if (m < 1 || lde < m) return fail(who, ": lde < m");
  if (short_j) return fail(who, short_j);
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  if (reinterpret_cast<uintptr_t>(J) % el || reinterpret_cast<uintptr_t>(e) % el) return fail(who, ": pointer not aligned");
  const int64_t total = ((int64_t)n_terms * B + 255) / 256;
  if (total > (int64_t)INT32_MAX) return fail(who, ": grid limit exceeded (n_terms * B)");
  *blocks = (unsigned)total;
  return 0;
}

}  // namespace thx
