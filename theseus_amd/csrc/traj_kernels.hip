// 2D motion planning (examples/motion_planning_2d.py of the reference): the cost family of a trajectory objective --
// Collision2D on Point2 (theseus/embodied/collision/collision.py:44-73 over SignedDistanceField2D.signed_distance,
// signed_distance_field.py:163-241), GPMotionModel with GPCostWeight (theseus/embodied/motionmodel/double_integrator.py:
// 48-80, 131-170) and Difference priors on 2-dof Euclidean variables (theseus/embodied/misc/local_cost_fn.py:16-75) --
// evaluated by ONE launch instead of one torch call chain per cost object.
//
// thx_traj2_eval: one thread per (term, problem), problems fastest; the host sorts the terms by kind, so a wave takes one
// branch except where two kinds meet.  A thread reads its variables from the (B, n) state and the term's aux data through
// the term table, and writes the WEIGHTED Jacobian blocks and the weighted error where thx_block_assemble's term tables point.
// thx_traj2_error: one workgroup per problem; thread i sums the squares of terms i, i + 256, ... in fp64, then a fixed-order
// tree over the workgroup -- deterministic, one launch.
//
// The geometric part (cell coordinates, bounds test, bilinear value, distance > eps test) runs in the run's dtype with
// contraction off and in the reference's operation order, so a kink lands where the torch classes put it.
#include "common.cuh"

namespace thx {

constexpr int kTrajErrThreads = 256;

template <typename T>
__device__ inline T aux_at(const thx_traj2_term& tm, int k, int b, int i = 0) {
  return static_cast<const T*>(tm.aux[k])[(int64_t)b * tm.aux_bstride[k] + i];
}

// Collision2D: weighted error (1) and, when J != nullptr, the weighted 1 x 2 block.
template <typename T>
__device__ inline T collision_term(const thx_traj2_term& tm, const T* __restrict__ x, int b, T* __restrict__ J) {
#pragma clang fp contract(off)
  const T px = x[tm.col[0]], py = x[tm.col[0] + 1];
  const T* sdf = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T ox = aux_at<T>(tm, 1, b, 0), oy = aux_at<T>(tm, 1, b, 1);
  const T cell = aux_at<T>(tm, 2, b), eps = aux_at<T>(tm, 3, b), w = aux_at<T>(tm, 4, b);
  const int R = tm.rows, C = tm.cols;
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
  T dist = hrd * hcd * sll + lrd * hcd * shl + hrd * lcd * slh + lrd * lcd * shh;   // :215-220
  T j1 = (hrd * (slh - sll) + lrd * (shh - shl)) / cell;                             // :231-238
  T j2 = (hcd * (shl - sll) + lcd * (shh - slh)) / cell;
  if (oob) dist = (T)0, j1 = (T)0, j2 = (T)0;   // sdf_boundary_value = 0 (collision.py:40-42)
  T err = eps - dist;                           // collision.py:61-62
  if (err < (T)0) err = (T)0;
  if (dist > eps) j1 = (T)0, j2 = (T)0;         // :71-73
  if (J) {
    J[0] = -j1 * w;
    J[1] = -j2 * w;
  }
  return err * w;
}

// GPMotionModel: weighted error (4) and, when J != nullptr, the four weighted 4 x 2 blocks (pose1, vel1, pose2, vel2), block s at
// J + s * jstep.
template <typename T>
__device__ inline void gp_term(const thx_traj2_term& tm, const T* __restrict__ x, int b, T* __restrict__ e, T* __restrict__ J,
                               int64_t jstep) {
  const T dt = aux_at<T>(tm, 0, b), dtw = aux_at<T>(tm, 1, b);
  // (the reference factorises W^T: of a Qc_inv that is not exactly symmetric it reads the UPPER triangle)
  const T q11 = aux_at<T>(tm, 2, b, 0), q21 = aux_at<T>(tm, 2, b, 1), q22 = aux_at<T>(tm, 2, b, 3);
  // U = chol(W)^T, W = M (x) Qc_inv (double_integrator.py:131-152) = chol(M)^T (x) chol(Qc_inv)^T
  const T m11 = (T)12 / (dtw * dtw * dtw), m21 = (T)-6 / (dtw * dtw), m22 = (T)4 / dtw;
  const T a = sqrt(m11), bb = m21 / a, c = sqrt(m22 - bb * bb);
  const T l11 = sqrt(q11), l21 = q21 / l11, l22 = sqrt(q22 - l21 * l21);
  // rows of U: [a Lq^T, bb Lq^T ; 0, c Lq^T],  Lq^T = [[l11, l21], [0, l22]]
  const T U[4][4] = {{a * l11, a * l21, bb * l11, bb * l21},
                     {(T)0, a * l22, (T)0, bb * l22},
                     {(T)0, (T)0, c * l11, c * l21},
                     {(T)0, (T)0, (T)0, c * l22}};
  const T* p1 = x + tm.col[0];
  const T* v1 = x + tm.col[1];
  const T* p2 = x + tm.col[2];
  const T* v2 = x + tm.col[3];
  const T r[4] = {p2[0] - p1[0] - dt * v1[0], p2[1] - p1[1] - dt * v1[1], v2[0] - v1[0], v2[1] - v1[1]};   // :53-56
  for (int i = 0; i < 4; ++i) e[i] = U[i][0] * r[0] + U[i][1] * r[1] + U[i][2] * r[2] + U[i][3] * r[3];
  if (!J) return;
  // :72-80 with Vector.local's Jacobians (-I, I): d r / d pose1 = [-I; 0], vel1 = [-dt I; -I], pose2 = [I; 0], vel2 = [0; I]
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 2; ++k) {
      J[0 * jstep + 2 * i + k] = -U[i][k];
      J[1 * jstep + 2 * i + k] = -dt * U[i][k] - U[i][2 + k];
      J[2 * jstep + 2 * i + k] = U[i][k];
      J[3 * jstep + 2 * i + k] = U[i][2 + k];
    }
}

// Difference on a 2-dof Euclidean variable: e = (x - target) * w, J = diag(w).
template <typename T>
__device__ inline void prior_term(const thx_traj2_term& tm, const T* __restrict__ x, int b, T* __restrict__ e, T* __restrict__ J) {
  const T w0 = aux_at<T>(tm, 1, b, 0), w1 = tm.wdim == 2 ? aux_at<T>(tm, 1, b, 1) : w0;
  e[0] = (x[tm.col[0]] - aux_at<T>(tm, 0, b, 0)) * w0;
  e[1] = (x[tm.col[0] + 1] - aux_at<T>(tm, 0, b, 1)) * w1;
  if (J) {
    J[0] = w0, J[1] = (T)0;
    J[2] = (T)0, J[3] = w1;
  }
}

__device__ inline int term_dim(int kind) { return kind == THX_TRAJ2_COLLISION ? 1 : (kind == THX_TRAJ2_GP ? 4 : 2); }
__device__ inline int term_vars(int kind) { return kind == THX_TRAJ2_GP ? 4 : 1; }

// every column a term reads lies inside the state, and the kind is one of the three
__device__ inline bool term_reads_ok(const thx_traj2_term& tm, int n) {
  if (tm.kind < THX_TRAJ2_COLLISION || tm.kind > THX_TRAJ2_PRIOR) return false;
  for (int s = 0; s < term_vars(tm.kind); ++s)
    if (tm.col[s] < 0 || tm.col[s] + 2 > n) return false;
  if (tm.kind == THX_TRAJ2_COLLISION && (tm.rows < 1 || tm.cols < 1)) return false;
  return true;
}

template <typename T>
__global__ void __launch_bounds__(256)
traj2_eval_kernel(const thx_traj2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int64_t ldx, int n,
                  T* __restrict__ J, int64_t j_total, T* __restrict__ e, int64_t lde, int m, int B) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_traj2_term tm = terms[t];
  if (!term_reads_ok(tm, n)) return;
  const int dim = term_dim(tm.kind), nv = term_vars(tm.kind);
  if (tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)2 * dim * nv > j_total) return;
  const T* xb = x + (int64_t)b * ldx;
  T* eb = e + (int64_t)b * lde + tm.row0;
  T* Jb = J + tm.j_off * B + (int64_t)2 * dim * b;
  if (tm.kind == THX_TRAJ2_COLLISION) {
    eb[0] = collision_term<T>(tm, xb, b, Jb);
  } else if (tm.kind == THX_TRAJ2_GP) {
    T ev[4];
    gp_term<T>(tm, xb, b, ev, Jb, (int64_t)8 * B);
    for (int i = 0; i < 4; ++i) eb[i] = ev[i];
  } else {
    T ev[2];
    prior_term<T>(tm, xb, b, ev, Jb);
    eb[0] = ev[0], eb[1] = ev[1];
  }
}

template <typename T>
__global__ void __launch_bounds__(kTrajErrThreads)
traj2_error_kernel(const thx_traj2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int64_t ldx, int n,
                   T* __restrict__ err) {
  __shared__ double part[kTrajErrThreads];
  const int b = blockIdx.x;
  const T* xb = x + (int64_t)b * ldx;
  double acc = 0.0;
  for (int t = threadIdx.x; t < n_terms; t += kTrajErrThreads) {
    const thx_traj2_term tm = terms[t];
    if (!term_reads_ok(tm, n)) continue;
    if (tm.kind == THX_TRAJ2_COLLISION) {
      const double v = (double)collision_term<T>(tm, xb, b, nullptr);
      acc += v * v;
    } else if (tm.kind == THX_TRAJ2_GP) {
      T ev[4];
      gp_term<T>(tm, xb, b, ev, nullptr, 0);
      for (int i = 0; i < 4; ++i) acc += (double)ev[i] * (double)ev[i];
    } else {
      T ev[2];
      prior_term<T>(tm, xb, b, ev, nullptr);
      acc += (double)ev[0] * (double)ev[0] + (double)ev[1] * (double)ev[1];
    }
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kTrajErrThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) err[b] = (T)(0.5 * part[0]);
}

// what both exports check on the host before any launch
inline int traj2_check(const char* who, const void* terms, int32_t n_terms, const void* x, int64_t ldx, int32_t n, int32_t B, int dtype) {
  if (!terms || !x) return fail(who, ": null pointer");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (n_terms < 1) return fail(who, ": n_terms < 1");
  if (B < 1) return fail(who, ": empty batch");
  if (n < 2) return fail(who, ": n < 2");
  if (ldx < n) return fail(who, ": ldx < n");
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  if (reinterpret_cast<uintptr_t>(terms) % 8 || reinterpret_cast<uintptr_t>(x) % el) return fail(who, ": pointer not aligned");
  return 0;
}

}  // namespace thx

using namespace thx;

extern "C" int thx_traj2_eval(const thx_traj2_term* terms, int32_t n_terms, const void* x, int64_t ldx, int32_t n, void* J,
                              int64_t j_total, void* e, int64_t lde, int32_t m, int32_t B, int dtype, void* stream) {
  const char* who = "thx_traj2_eval";
  if (!J || !e) return fail(who, ": null pointer");
  if (int rc = traj2_check(who, terms, n_terms, x, ldx, n, B, dtype)) return rc;
  if (m < 1 || lde < m) return fail(who, ": lde < m");
  if (j_total < 2) return fail(who, ": j_total < 2");
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  if (reinterpret_cast<uintptr_t>(J) % el || reinterpret_cast<uintptr_t>(e) % el) return fail(who, ": pointer not aligned");
  const int64_t total = (int64_t)n_terms * B;
  if ((total + 255) / 256 > (int64_t)INT32_MAX) return fail(who, ": grid limit exceeded (n_terms * B)");
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(traj2_eval_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, (const float*)x,
                                  ldx, n, (float*)J, j_total, (float*)e, lde, m, B),
               hipLaunchKernelGGL(traj2_eval_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, (const double*)x,
                                  ldx, n, (double*)J, j_total, (double*)e, lde, m, B));
  return check_launch(who);
}

extern "C" int thx_traj2_error(const thx_traj2_term* terms, int32_t n_terms, const void* x, int64_t ldx, int32_t n, void* err,
                               int32_t B, int dtype, void* stream) {
  const char* who = "thx_traj2_error";
  if (!err) return fail(who, ": null pointer");
  if (int rc = traj2_check(who, terms, n_terms, x, ldx, n, B, dtype)) return rc;
  if (reinterpret_cast<uintptr_t>(err) % (dtype == THX_F32 ? 4 : 8)) return fail(who, ": pointer not aligned");
  const dim3 grid((unsigned)B), block(kTrajErrThreads);   // (B <= INT32_MAX: within the grid limit of the x dimension)
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(traj2_error_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, (const float*)x,
                                  ldx, n, (float*)err),
               hipLaunchKernelGGL(traj2_error_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms,
                                  (const double*)x, ldx, n, (double*)err));
  return check_launch(who);
}
