// What the fused cost families (traj_kernels.hip, push_kernels.hip + push_vjp_kernels.hip, trajse2_kernels.hip + trajse2_vjp_kernels.hip, homog_kernels.hip +
// homog_vjp_kernels.hip, kin_kernels.hip + kin_vjp_kernels.hip) share: a family evaluates a whole objective from a table of 128-byte terms (thx_traj2_term,
// thx_push2_term, thx_trajse2_term of include/theseus_hip.h: the same layout, the variable field named by the family).
// Here: the per-term aux accessor, the bilinear signed-distance lookup and the backward of a Collision2D term on it, the fixed-order reduction of a *_error kernel, stage B of a
// *_vjp export on its per-(term, problem) records (vjp_reduce_kernel for the small tensors; vjp_scatter_kernel + vjp_grid_out_kernel
// for 2-D grids, templated on the term type and the kind that reads the grid) and the host checks and stage-B launches of the
// exports.  The term functions, stage A, the *_eval / *_error __global__ functions and the exports stay with the family.
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
// ... what a backward kernel needs on top of the value: the clamped corner indices, the unclamped corner coordinates, the four
// corner values and the in-grid test
template <typename T>
struct SdfCells {
  int lri, lci, hri, hci;
  T lr, lc, sll, shl, slh, shh;
  bool oob;
};

template <typename T>
__device__ __forceinline__ void sdf_bilinear_cells(const T* __restrict__ sdf, int R, int C, T ox, T oy, T cell, T px, T py, T& dist,
                                                   T& j1, T& j2, SdfCells<T>& k) {
#pragma clang fp contract(off)
  // signed_distance_field.py:179-187
  k.oob = (px < ox) || (px > (ox + (T)(C - 1.0) * cell)) || (py < oy) || (py > (oy + (T)(R - 1.0) * cell));
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
  if (k.oob) dist = (T)0, j1 = (T)0, j2 = (T)0;
  k.lri = lri, k.lci = lci, k.hri = hri, k.hci = hci;
  k.lr = lr, k.lc = lc, k.sll = sll, k.shl = shl, k.slh = slh, k.shh = shh;
}

template <typename T>
__device__ __forceinline__ void sdf_bilinear(const T* __restrict__ sdf, int R, int C, T ox, T oy, T cell, T px, T py, T& dist, T& j1,
                                             T& j2) {
  SdfCells<T> k;
  sdf_bilinear_cells<T>(sdf, R, C, ox, oy, cell, px, py, dist, j1, j2, k);
}

// The backward of a Collision2D term (thx_traj2_vjp, thx_trajse2_vjp): phi = w^2 s (eps - d), s = j1 u_x + j2 u_y, with (u_x, u_y)
// the cotangent of the looked-up point (px, py) in the world frame.  The branches are the forward's, in T; the derivatives in fp64.
// Record entries through out.put(k, v): 0-3 d / d corner value (ll, hl, lh, hh), 4-7 their cell indices row * cols + col, 8-9 origin,
// 10 cell size, 11 cost_eps, 12 weight.  -> false, and nothing is written, outside the grid or where the distance exceeds eps (the
// error and the block are constants there)
template <typename T, typename Term, typename Out>
__device__ __forceinline__ bool collision_vjp_at(const Term& tm, T px_t, T py_t, double ux, double uy, int b, const Out& out) {
  const T* sdf = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T eps_t = aux_at<T>(tm, 3, b), ox_t = aux_at<T>(tm, 1, b, 0), oy_t = aux_at<T>(tm, 1, b, 1), cell_t = aux_at<T>(tm, 2, b);
  T dist, j1, j2;
  SdfCells<T> k;
  sdf_bilinear_cells<T>(sdf, tm.rows, tm.cols, ox_t, oy_t, cell_t, px_t, py_t, dist, j1, j2, k);
  if (k.oob || dist > eps_t) return false;
  const double w = (double)aux_at<T>(tm, 4, b), eps = (double)eps_t, cell = (double)cell_t;
  const double col = ((double)px_t - (double)ox_t) / cell, row = ((double)py_t - (double)oy_t) / cell;
  const double lr = (double)k.lr, lc = (double)k.lc;
  const double hrd = lr + 1.0 - row, hcd = lc + 1.0 - col, lrd = row - lr, lcd = col - lc;
  const double sll = (double)k.sll, shl = (double)k.shl, slh = (double)k.slh, shh = (double)k.shh;
  const double d = hrd * hcd * sll + lrd * hcd * shl + hrd * lcd * slh + lrd * lcd * shh;
  const double dc = hrd * (slh - sll) + lrd * (shh - shl), dr = hcd * (shl - sll) + lcd * (shh - slh);   // d d / d col, d d / d row
  const double s = (dc * ux + dr * uy) / cell, gap = eps - d, w2 = w * w;
  // d s / d corner from the j1 / j2 formulas; the corner's bilinear weight is d d / d corner
  out.put(0, w2 * (gap * (-hrd * ux - hcd * uy) / cell - s * hrd * hcd));
  out.put(1, w2 * (gap * (-lrd * ux + hcd * uy) / cell - s * lrd * hcd));
  out.put(2, w2 * (gap * (hrd * ux - lcd * uy) / cell - s * hrd * lcd));
  out.put(3, w2 * (gap * (lrd * ux + lcd * uy) / cell - s * lrd * lcd));
  out.put(4, (double)((int64_t)k.lri * tm.cols + k.lci));
  out.put(5, (double)((int64_t)k.hri * tm.cols + k.lci));
  out.put(6, (double)((int64_t)k.lri * tm.cols + k.hci));
  out.put(7, (double)((int64_t)k.hri * tm.cols + k.hci));
  // through col = (px - ox) / cell, row = (py - oy) / cell; the only second derivative of the bilinear form is the mixed one
  const double mixed = sll - shl - slh + shh;
  const double pcol = w2 * (gap * mixed * uy / cell - s * dc), prow = w2 * (gap * mixed * ux / cell - s * dr);
  out.put(8, -pcol / cell);
  out.put(9, -prow / cell);
  out.put(10, -(pcol * col + prow * row + w2 * gap * s) / cell);   // (the last: j1, j2 divide by the cell size themselves)
  out.put(11, w2 * s);
  out.put(12, 2.0 * w * s * gap);
  return true;
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

// where one (term, problem) of a stage A kernel stores its record of REC doubles: entry k at p[k * B]
template <int REC>
struct RecOutT {
  double* __restrict__ p;
  int64_t B;
  __device__ __forceinline__ void put(int k, double v) const { p[k * B] = v; }
  __device__ __forceinline__ void zeros(int from, int to = REC) const {
    for (int k = from; k < to; ++k) p[k * B] = 0.0;
  }
  // d phi / d row weights from the n per-row values: n entries for a DiagonalCostWeight, their sum (and zeros) for a ScaleCostWeight
  template <int n = 3>
  __device__ __forceinline__ void weights(int k, int wdim, const double* gw) const {
    double sum = gw[0];
#pragma unroll
    for (int i = 1; i < n; ++i) sum += gw[i];
    put(k, wdim == n ? gw[0] : sum);
#pragma unroll
    for (int i = 1; i < n; ++i) put(k + i, wdim == n ? gw[i] : 0.0);
  }
};

// The small-tensor stage of a family's VJP export (thx_traj2_vjp, thx_push2_vjp, thx_homog_vjp, thx_kin_vjp): rec holds REC doubles per (term, problem), entry k
// of term t of problem b at rec[(t * REC + k) * B + b].  Workgroup = (tensor, problem), or the tensor when it is shared; fixed-order
// sums in fp64
template <typename T>
__device__ __forceinline__ void vjp_reduce(const double* __restrict__ rec, const int REC, int n_terms,
                                           const thx_traj2_grad_tensor* __restrict__ tensors,
                                           const thx_traj2_grad_pair* __restrict__ pairs, int n_pairs, T* __restrict__ out,
                                           int64_t out_elems, int B) {
  __shared__ double part[256];
  const int g = (int)(blockIdx.x / (unsigned)B), b = (int)(blockIdx.x % (unsigned)B);
  const thx_traj2_grad_tensor tg = tensors[g];
  // (everything below is uniform over the workgroup)
  if (tg.shared && b > 0) return;
  if (tg.pair_begin < 0 || tg.pair_end < tg.pair_begin || tg.pair_end > n_pairs || tg.count < 1 || tg.count > REC) return;
  const int64_t o0 = tg.out_off + (tg.shared ? 0 : (int64_t)b * tg.count);
  if (tg.out_off < 0 || o0 + tg.count > out_elems) return;
  const int64_t contributions = (int64_t)(tg.pair_end - tg.pair_begin) * (tg.shared ? B : 1);
  for (int j = 0; j < tg.count; ++j) {
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < contributions; c += 256) {
      const thx_traj2_grad_pair pr = pairs[tg.pair_begin + (tg.shared ? c / B : c)];
      const int bb = tg.shared ? (int)(c % B) : b;
      if (pr.term < 0 || pr.term >= n_terms || pr.entry < 0 || pr.entry + tg.count > REC) continue;
      acc += rec[((int64_t)pr.term * REC + pr.entry + j) * B + bb];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[o0 + j] = (T)part[0];
    __syncthreads();
  }
}
template <typename T, int REC>
__global__ void __launch_bounds__(256)
vjp_reduce_kernel(const double* __restrict__ rec, int n_terms, const thx_traj2_grad_tensor* __restrict__ tensors,
                        const thx_traj2_grad_pair* __restrict__ pairs, int n_pairs, T* __restrict__ out, int64_t out_elems, int B) {
  vjp_reduce<T>(rec, REC, n_terms, tensors, pairs, n_pairs, out, out_elems, B);
}
// ... for a family whose record width is known at run time only (thx_kin_vjp: it grows with the robot's degrees of freedom)
template <typename T>
__global__ void __launch_bounds__(256)
vjp_reduce_strided_kernel(const double* __restrict__ rec, int rec_stride, int n_terms, const thx_traj2_grad_tensor* __restrict__ tensors,
                          const thx_traj2_grad_pair* __restrict__ pairs, int n_pairs, T* __restrict__ out, int64_t out_elems, int B) {
  vjp_reduce<T>(rec, rec_stride, n_terms, tensors, pairs, n_pairs, out, out_elems, B);
}

constexpr int kSortChunk = THX_TRAJ2_SORT_CHUNK;   // (cell, value) pairs the grid scatter sorts at a time

// The grid stage of a family's VJP export (thx_traj2_vjp, thx_push2_vjp): workgroup = (problem, grid).  The four (cell, value)
// pairs (record entries 4-7 and 0-3) of each term of kind GRID_KIND on this grid go through LDS a chunk at a time: a bitonic network
// sorts the chunk by (cell, position in the list) -- a unique key, so the order of equal cells is fixed --, the head of each run of equal cells sums the run in that order and adds it into the problem's fp64 grid.  Within a
// chunk a cell has one head; chunks follow one another behind a barrier, so a cell two chunks touch is updated in chunk order.
template <typename Term, int GRID_KIND, int REC>
__global__ void __launch_bounds__(256)
vjp_scatter_kernel(const double* __restrict__ rec, const Term* __restrict__ terms, int n_terms,
                   const thx_traj2_grad_grid* __restrict__ grids, const int32_t* __restrict__ grid_terms, int n_grid_terms,
                   double* __restrict__ work, int64_t work_elems, int B) {
  __shared__ unsigned long long key[kSortChunk];
  __shared__ double val[kSortChunk];
  constexpr unsigned long long kPad = ~0ull;
  const int b = blockIdx.x;
  const thx_traj2_grad_grid gd = grids[blockIdx.y];
  const int64_t cells = (int64_t)gd.rows * gd.cols;
  if (gd.rows < 1 || gd.cols < 1 || cells > INT32_MAX || gd.term_begin < 0 || gd.term_end < gd.term_begin || gd.term_end > n_grid_terms)
    return;
  if (gd.work_off < 0 || gd.work_off + cells * B > work_elems) return;
  double* gg = work + gd.work_off + cells * b;
  for (int64_t c = threadIdx.x; c < cells; c += 256) gg[c] = 0.0;
  __syncthreads();
  const int64_t n_src = (int64_t)4 * (gd.term_end - gd.term_begin);
  for (int64_t base = 0; base < n_src; base += kSortChunk) {
    for (int i = threadIdx.x; i < kSortChunk; i += 256) {
      const int64_t p = base + i;
      unsigned long long kk = kPad;
      double v = 0.0;
      if (p < n_src) {
        const int t = grid_terms[gd.term_begin + p / 4], c = (int)(p % 4);
        if (t >= 0 && t < n_terms && terms[t].kind == GRID_KIND && terms[t].rows == gd.rows && terms[t].cols == gd.cols) {
          const double cell = rec[((int64_t)t * REC + 4 + c) * B + b];
          if (cell >= 0.0 && cell < (double)cells) {
            kk = ((unsigned long long)cell << 32) | (unsigned long long)i;   // (i: the position within the chunk, p - base)
            v = rec[((int64_t)t * REC + c) * B + b];
          }
        }
      }
      key[i] = kk, val[i] = v;
    }
    __syncthreads();
    for (int k = 2; k <= kSortChunk; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < kSortChunk; i += 256) {
          const int l = i ^ j;
          if (l > i) {
            const unsigned long long a = key[i], c = key[l];
            if ((a > c) == ((i & k) == 0)) {
              const double va = val[i];
              key[i] = c, key[l] = a, val[i] = val[l], val[l] = va;
            }
          }
        }
        __syncthreads();
      }
    for (int i = threadIdx.x; i < kSortChunk; i += 256) {
      const unsigned long long a = key[i];
      if (a == kPad || (i > 0 && (key[i - 1] >> 32) == (a >> 32))) continue;   // padding, or inside a run
      double acc = 0.0;
      for (int q = i; q < kSortChunk && (key[q] >> 32) == (a >> 32); ++q) acc += val[q];
      gg[a >> 32] += acc;
    }
    __syncthreads();
  }
}

// ... and out of the fp64 grids: one thread per (problem, cell), cells fastest; a shared grid is summed over the problems in index order
template <typename T>
__global__ void __launch_bounds__(256)
vjp_grid_out_kernel(const double* __restrict__ work, int64_t work_elems, const thx_traj2_grad_grid* __restrict__ grids,
                    int max_cells, T* __restrict__ out, int64_t out_elems, int B) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)max_cells * B) return;
  const int b = (int)(gid / max_cells);
  const int64_t c = gid % max_cells;
  const thx_traj2_grad_grid gd = grids[blockIdx.y];
  const int64_t cells = (int64_t)gd.rows * gd.cols;
  if (gd.rows < 1 || gd.cols < 1 || c >= cells || (gd.shared && b > 0)) return;
  if (gd.work_off < 0 || gd.work_off + cells * B > work_elems || gd.out_off < 0) return;
  const double* gg = work + gd.work_off;
  if (gd.shared) {
    if (gd.out_off + cells > out_elems) return;
    double acc = 0.0;
    for (int bb = 0; bb < B; ++bb) acc += gg[cells * bb + c];
    out[gd.out_off + c] = (T)acc;
  } else {
    if (gd.out_off + cells * B > out_elems) return;
    out[gd.out_off + cells * b + c] = (T)gg[cells * b + c];
  }
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

// ... and what a *_vjp export with a thx_traj2_grad_plan checks after family_check and its own sizes: the plan, the alignment of the
// cotangent, the record and the outputs, the grids of both stages.  -> the grid of stage A in ``term_blocks``
inline int family_check_vjp(const char* who, const void* u, const double* rec, const thx_traj2_grad_plan& p, const void* grad_out,
                            const double* grid_work, int32_t n_terms, int32_t B, int dtype, unsigned* term_blocks) {
  if (p.n_tensors < 0 || p.n_pairs < 0 || p.n_grids < 0 || p.n_grid_terms < 0 || p.max_cells < 0 || p.out_elems < 1 || p.work_elems < 0)
    return fail(who, ": negative size in the plan");
  if ((p.n_tensors > 0 && (!p.tensors || !p.pairs)) || (p.n_grids > 0 && (!p.grids || !p.grid_terms || !grid_work || p.max_cells < 1)))
    return fail(who, ": null pointer in the plan");
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  if (at(u) % el || at(grad_out) % el || at(rec) % 8 || at(grid_work) % 8 || at(p.tensors) % 8 || at(p.pairs) % 4 || at(p.grids) % 8 ||
      at(p.grid_terms) % 4)
    return fail(who, ": pointer not aligned");
  const int64_t blocks = ((int64_t)n_terms * B + 255) / 256, out_blocks = ((int64_t)p.max_cells * B + 255) / 256;
  if (blocks > (int64_t)INT32_MAX || (int64_t)p.n_tensors * B > (int64_t)INT32_MAX || out_blocks > (int64_t)INT32_MAX || p.n_grids > 65535)
    return fail(who, ": grid limit exceeded (n_terms * B, tensors * B, cells * B or the number of grids)");
  *term_blocks = (unsigned)blocks;
  return 0;
}

// stage B of such an export on the records stage A wrote: the small tensors, then the grids read by the terms of kind GRID_KIND
template <typename Term, int GRID_KIND, int REC>
inline int family_vjp_stage_b(const double* rec, const Term* terms, int32_t n_terms, const thx_traj2_grad_plan& p, void* grad_out,
                               double* grid_work, int32_t B, int dtype, hipStream_t s) {
  const dim3 block(256);
  if (p.n_tensors > 0) {
    const dim3 grid((unsigned)((int64_t)p.n_tensors * B));
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL((vjp_reduce_kernel<float, REC>), grid, block, 0, s, rec, n_terms, p.tensors, p.pairs, p.n_pairs,
                                    (float*)grad_out, p.out_elems, B),
                 hipLaunchKernelGGL((vjp_reduce_kernel<double, REC>), grid, block, 0, s, rec, n_terms, p.tensors, p.pairs, p.n_pairs,
                                    (double*)grad_out, p.out_elems, B));
  }
  if (p.n_grids > 0) {
    hipLaunchKernelGGL((vjp_scatter_kernel<Term, GRID_KIND, REC>), dim3((unsigned)B, (unsigned)p.n_grids), block, 0, s, rec, terms,
                       n_terms, p.grids, p.grid_terms, p.n_grid_terms, grid_work, p.work_elems, B);
    const dim3 grid((unsigned)(((int64_t)p.max_cells * B + 255) / 256), (unsigned)p.n_grids);
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL(vjp_grid_out_kernel<float>, grid, block, 0, s, grid_work, p.work_elems, p.grids, p.max_cells,
                                    (float*)grad_out, p.out_elems, B),
                 hipLaunchKernelGGL(vjp_grid_out_kernel<double>, grid, block, 0, s, grid_work, p.work_elems, p.grids, p.max_cells,
                                    (double*)grad_out, p.out_elems, B));
  }
  return 0;
}

}  // namespace thx
