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

// ---- thx_traj2_vjp: the gradient of u^T g, g = -sum_t J_t^T e_t at a detached state, w.r.t. the auxiliary tensors ------------------
// Per term phi_t = -(sum_s J_s u_s) . e_t; floor(), the in-grid test and the distance > eps test are constants, as in the torch
// classes.  Stage A (traj2_vjp_terms_kernel) writes each term's partial derivatives, stage B gathers them per tensor
// or scatters them into the grids (vjp_reduce_kernel, vjp_scatter_kernel + vjp_grid_out_kernel of term_family.cuh).
constexpr int kRec = THX_TRAJ2_REC;

// Collision2D on a Point2: collision_vjp_at of term_family.cuh at the point itself, with the point's own cotangent columns
struct RecArray {
  double* o;
  __device__ __forceinline__ void put(int k, double v) const { o[k] = v; }
};
template <typename T>
__device__ inline void collision_vjp(const thx_traj2_term& tm, const T* __restrict__ x, const T* __restrict__ u, int b, double* o) {
  collision_vjp_at<T>(tm, x[tm.col[0]], x[tm.col[0] + 1], (double)u[tm.col[0]], (double)u[tm.col[0] + 1], b, RecArray{o});
}

// GPMotionModel: phi = -rho^T W r, W = M(dt_w) (x) Qc_inv, rho = [u_p2 - u_p1 - dt u_v1 ; u_v2 - u_v1]; no Cholesky is differentiated.
// For a Qc_inv that is not symmetric the torch twin decides what each derivative sees: its Cholesky returns the symmetrised
// cotangent, so d / d Qc_inv has the off-diagonal split evenly and d / d dt_w (through the twin's blocks 12 dt^-3 Qc_inv, ...) sees
// (Qc_inv + Qc_inv^T) / 2; d / d dt sees the matrix that Cholesky factorises (below).
template <typename T>
__device__ inline void gp_vjp(const thx_traj2_term& tm, const T* __restrict__ x, const T* __restrict__ u, int b, double* o) {
  const double dt = (double)aux_at<T>(tm, 0, b), dtw = (double)aux_at<T>(tm, 1, b);
  const double q00 = (double)aux_at<T>(tm, 2, b, 0), q01 = (double)aux_at<T>(tm, 2, b, 1), q10 = (double)aux_at<T>(tm, 2, b, 2),
               q11 = (double)aux_at<T>(tm, 2, b, 3);
  const double M[2][2] = {{12.0 / (dtw * dtw * dtw), -6.0 / (dtw * dtw)}, {-6.0 / (dtw * dtw), 4.0 / dtw}};
  const double dM[2][2] = {{-36.0 / (dtw * dtw * dtw * dtw), 12.0 / (dtw * dtw * dtw)}, {12.0 / (dtw * dtw * dtw), -4.0 / (dtw * dtw)}};
  double r[2][2], rho[2][2], v1[2], uv1[2];
  for (int i = 0; i < 2; ++i) {
    v1[i] = (double)x[tm.col[1] + i], uv1[i] = (double)u[tm.col[1] + i];
    r[0][i] = (double)x[tm.col[2] + i] - (double)x[tm.col[0] + i] - dt * v1[i];
    r[1][i] = (double)x[tm.col[3] + i] - v1[i];
    rho[0][i] = (double)u[tm.col[2] + i] - (double)u[tm.col[0] + i] - dt * uv1[i];
    rho[1][i] = (double)u[tm.col[3] + i] - uv1[i];
  }
  auto form = [](const double* a, double m00, double m01, double m10, double m11, const double* c) {   // a^T [[m00, m01], [m10, m11]] c
    return a[0] * (m00 * c[0] + m01 * c[1]) + a[1] * (m10 * c[0] + m11 * c[1]);
  };
  // the matrix the twin's Cholesky factorises is the lower triangle of W^T completed symmetrically: its diagonal blocks see the
  // upper triangle of Qc_inv, the block below the diagonal all of Qc_inv^T (and the one above, by symmetry, Qc_inv)
  const double qs = 0.5 * (q01 + q10);
  double g_dtw = 0.0, G[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  const double g_dt = M[0][0] * (form(uv1, q00, q01, q01, q11, r[0]) + form(rho[0], q00, q01, q01, q11, v1)) +
         M[0][1] * (form(uv1, q00, q01, q10, q11, r[1]) + form(rho[1], q00, q10, q01, q11, v1));
  for (int a = 0; a < 2; ++a) {
    for (int c = 0; c < 2; ++c) {
      g_dtw -= dM[a][c] * form(rho[a], q00, qs, qs, q11, r[c]);
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) G[i][j] -= M[a][c] * rho[a][i] * r[c][j];
    }
  }
  o[0] = g_dt, o[1] = g_dtw;
  o[2] = G[0][0], o[3] = o[4] = 0.5 * (G[0][1] + G[1][0]), o[5] = G[1][1];
}

// Difference: phi = -sum_i u_i w_i^2 (x_i - t_i)
template <typename T>
__device__ inline void prior_vjp(const thx_traj2_term& tm, const T* __restrict__ x, const T* __restrict__ u, int b, double* o) {
  double gw[2];
  for (int i = 0; i < 2; ++i) {
    const double w = (double)aux_at<T>(tm, 1, b, tm.wdim == 2 ? i : 0), ui = (double)u[tm.col[0] + i];
    o[i] = ui * w * w;
    gw[i] = -2.0 * ui * w * ((double)x[tm.col[0] + i] - (double)aux_at<T>(tm, 0, b, i));
  }
  if (tm.wdim == 2) o[2] = gw[0], o[3] = gw[1];
  else o[2] = gw[0] + gw[1];
}

// stage A: traj2_eval_kernel's map and guards; every (term, problem) writes its whole record, zeros where the term is skipped
template <typename T>
__global__ void __launch_bounds__(256)
traj2_vjp_terms_kernel(const thx_traj2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int64_t ldx, int n,
                       const T* __restrict__ u, int64_t ldu, int m, int64_t j_total, double* __restrict__ rec, int B) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_traj2_term tm = terms[t];
  double o[kRec];
  for (int k = 0; k < kRec; ++k) o[k] = 0.0;
  bool ok = term_reads_ok(tm, n);
  if (ok) {
    const int dim = term_dim(tm.kind), nv = term_vars(tm.kind);
    ok = !(tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)2 * dim * nv > j_total);
  }
  if (ok) {
    const T* xb = x + (int64_t)b * ldx;
    const T* ub = u + (int64_t)b * ldu;
    if (tm.kind == THX_TRAJ2_COLLISION) collision_vjp<T>(tm, xb, ub, b, o);
    else if (tm.kind == THX_TRAJ2_GP) gp_vjp<T>(tm, xb, ub, b, o);
    else prior_vjp<T>(tm, xb, ub, b, o);
  }
  for (int k = 0; k < kRec; ++k) rec[((int64_t)t * kRec + k) * B + b] = o[k];
}

// stage B, small tensors: vjp_reduce_kernel of term_family.cuh

// stage B, grids: vjp_scatter_kernel + vjp_grid_out_kernel of term_family.cuh

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

extern "C" int thx_traj2_vjp(const thx_traj2_term* terms, int32_t n_terms, const void* x, int64_t ldx, int32_t n, const void* u,
                             int64_t ldu, int32_t m, int64_t j_total, double* rec, const thx_traj2_grad_plan* plan, void* grad_out,
                             double* grid_work, int32_t B, int dtype, void* stream) {
  const char* who = "thx_traj2_vjp";
  if (int rc = family_check(who, !u || !rec || !plan || !grad_out, terms, n_terms, x, 1, B, dtype, traj2_bad_size(ldx, n))) return rc;
  if (ldu < n) return fail(who, ": ldu < n");
  if (m < 1 || j_total < 2) return fail(who, ": m < 1 or j_total < 2");
  const thx_traj2_grad_plan p = *plan;
  unsigned term_blocks = 0;
  if (int rc = family_check_vjp(who, u, rec, p, grad_out, grid_work, n_terms, B, dtype, &term_blocks)) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(traj2_vjp_terms_kernel<float>, dim3(term_blocks), block, 0, s, terms, n_terms,
                                  (const float*)x, ldx, n, (const float*)u, ldu, m, j_total, rec, B),
               hipLaunchKernelGGL(traj2_vjp_terms_kernel<double>, dim3(term_blocks), block, 0, s, terms, n_terms,
                                  (const double*)x, ldx, n, (const double*)u, ldu, m, j_total, rec, B));
  if (int rc = family_vjp_stage_b<thx_traj2_term, THX_TRAJ2_COLLISION, kRec>(rec, terms, n_terms, p, grad_out, grid_work, B, dtype, s)) return rc;
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
