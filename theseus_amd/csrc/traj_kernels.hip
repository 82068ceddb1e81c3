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
#include "term_family.cuh"

namespace thx {

// Collision2D: weighted error (1) and, when J != nullptr, the weighted 1 x 2 block.
template <typename T>
__device__ inline T collision_term(const thx_traj2_term& tm, const T* __restrict__ x, int b, T* __restrict__ J) {
#pragma clang fp contract(off)
  const T* sdf = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T eps = aux_at<T>(tm, 3, b), w = aux_at<T>(tm, 4, b);
  T dist, j1, j2;
  sdf_bilinear<T>(sdf, tm.rows, tm.cols, aux_at<T>(tm, 1, b, 0), aux_at<T>(tm, 1, b, 1), aux_at<T>(tm, 2, b), x[tm.col[0]],
                  x[tm.col[0] + 1], dist, j1, j2);   // (outside the grid: sdf_boundary_value = 0, collision.py:40-42)
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
__global__ void __launch_bounds__(kErrThreads)
traj2_error_kernel(const thx_traj2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int64_t ldx, int n,
                   T* __restrict__ err) {
  const int b = blockIdx.x;
  const T* xb = x + (int64_t)b * ldx;
  double acc = 0.0;
  for (int t = threadIdx.x; t < n_terms; t += kErrThreads) {
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
  store_half_sum(acc, err + b);
}

// the family's own size checks: the message of the first that fails
inline const char* traj2_bad_size(int64_t ldx, int32_t n) { return n < 2 ? ": n < 2" : (ldx < n ? ": ldx < n" : nullptr); }

}  // namespace thx

using namespace thx;

extern "C" int thx_traj2_eval(const thx_traj2_term* terms, int32_t n_terms, const void* x, int64_t ldx, int32_t n, void* J,
                              int64_t j_total, void* e, int64_t lde, int32_t m, int32_t B, int dtype, void* stream) {
  const char* who = "thx_traj2_eval";
  unsigned blocks = 0;
  if (int rc = family_check(who, !J || !e, terms, n_terms, x, 1, B, dtype, traj2_bad_size(ldx, n))) return rc;
  if (int rc = family_check_eval(who, J, j_total < 2 ? ": j_total < 2" : nullptr, e, lde, m, n_terms, B, dtype, &blocks)) return rc;
  const dim3 grid(blocks), block(256);
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
  if (int rc = family_check(who, !err, terms, n_terms, x, 1, B, dtype, traj2_bad_size(ldx, n))) return rc;
  if (reinterpret_cast<uintptr_t>(err) % (dtype == THX_F32 ? 4 : 8)) return fail(who, ": pointer not aligned");
  const dim3 grid((unsigned)B), block(kErrThreads);   // (B <= INT32_MAX: within the grid limit of the x dimension)
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(traj2_error_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, (const float*)x,
                                  ldx, n, (float*)err),
               hipLaunchKernelGGL(traj2_error_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms,
                                  (const double*)x, ldx, n, (double*)err));
  return check_launch(who);
}
