// The backward of the SE2 motion planner's implicit step (thx_trajse2_vjp): with g = -sum_t J_t^T e_t what thx_trajse2_eval +
// thx_block_assemble form at a detached state and u a cotangent of g, the gradient of u^T g w.r.t. the auxiliary tensors -- what
// autograd computes by walking the torch classes of theseus_amd/embodied.py and se2_torch.py back.  Per term
//   phi_t = -(sum_s J_s u_s) . e_t = -sum_i w_i^2 c_i e_i,   c = sum_s J_s^raw u_s,  e the raw error, w the row weights;
// for the GP kind phi = -rho^T W r with the full matrix W.
//
// Stage A (trajse2_vjp_terms_kernel): one thread per (term, problem), problems fastest, trajse2_eval_kernel's map and guards.  The term
// is read in place, a state record is one vector load, and a thread stores each record entry as soon as it has it (the stores of a
// wave are consecutive doubles): no record lives in registers or scratch.  A thread writes ONLY the entries its kind defines -- stage
// B reads the entries the plan's pairs name and entries 0-7 of collision terms, nothing else --, a compile-time count per kind; a term
// that fails a guard writes zeros to exactly those.  Every branch of the forward -- the in-grid test, floor, dist > eps, the hinge's
// strict comparisons, the Taylor switches of the SE2 log -- is decided in the run's dtype by the forward's own operations
// (sdf_bilinear_cells, lie_se2.cuh; the pragma below covers them); the derivatives are fp64 with that branch forced:
//   Collision2D        collision_vjp_at (term_family.cuh) at xy(pose) with the cotangent rotated into the world frame
//   GPMotionModel      closed forms in rho = [J0 u_p1 + Jlog u_p2 - dt u_v1 ; u_v2 - u_v1] and r; J0, Jlog are the forward's blocks
//                      (no auxiliary tensor enters them); no Cholesky is differentiated
//   Nonholonomic, HingeCost, Difference on a 3-vector, XYDifference    closed forms; the hinge selects by branches (limits of +-inf)
//   Difference on SE2  se2_prior_vjp (se2_vjp.cuh): Dual<double> through the error and Jlog
// Stage B: vjp_reduce_kernel, vjp_scatter_kernel and vjp_grid_out_kernel of term_family.cuh on the records.  No atomics.
#pragma clang fp contract(off)
#include "trajse2_family.cuh"
#include "se2_vjp.cuh"

namespace thx {

constexpr int kRec = THX_TRAJSE2_REC;
using RecOut = RecOutT<kRec>;

// the record entries a kind defines (a kind outside the seven: the whole record)
constexpr int kRecCollision = 13, kRecGp = 11, kRecNonholonomic = 1, kRecHinge = 12, kRecPriorSe2 = 7, kRecPriorVec = 6, kRecPriorXy = 4;
__device__ __forceinline__ int tse2_rec_count(int kind) {
  switch (kind) {
    case THX_TRAJSE2_COLLISION: return kRecCollision;
    case THX_TRAJSE2_GP: return kRecGp;
    case THX_TRAJSE2_NONHOLONOMIC: return kRecNonholonomic;
    case THX_TRAJSE2_HINGE: return kRecHinge;
    case THX_TRAJSE2_PRIOR_SE2: return kRecPriorSe2;
    case THX_TRAJSE2_PRIOR_VEC: return kRecPriorVec;
    case THX_TRAJSE2_PRIOR_XY: return kRecPriorXy;
    default: return kRec;
  }
}

template <typename T, int n>
__device__ __forceinline__ void tse2_weights64(const thx_trajse2_term& tm, int k, int b, double* w) {
  T wt[n];
  tse2_weights<T, n>(tm, k, b, wt);
#pragma unroll
  for (int i = 0; i < n; ++i) w[i] = (double)wt[i];
}

// record: collision_vjp_at's 13 entries; the forward's block is -(dd/dxy) [R, 0], so the point's cotangent is R u_xy
template <typename T>
__device__ __forceinline__ void tse2_collision_vjp(const thx_trajse2_term& tm, const SE2<T>& p, const T* __restrict__ ub, int b,
                                                   const RecOut& out) {
  const double u0 = (double)ub[3 * tm.var[0]], u1 = (double)ub[3 * tm.var[0] + 1], c = (double)p.c, s = (double)p.s;
  if (!collision_vjp_at<T>(tm, p.x, p.y, c * u0 - s * u1, s * u0 + c * u1, b, out)) out.zeros(0, kRecCollision);
}

// a^T Q c for a row-major 3 x 3 Q
__device__ __forceinline__ double form3(const double* a, const double* Q, const double* c) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) acc += a[i] * (Q[3 * i] * c[0] + Q[3 * i + 1] * c[1] + Q[3 * i + 2] * c[2]);
  return acc;
}

// record: 0 dt (the cost's), 1 dt (the weight's), 2-10 Qc_inv row major.  phi = -rho^T W r, W = M(dt_w) (x) Qc_inv.  For a Qc_inv
// that is not symmetric the torch twin decides what each derivative sees (gp_vjp of traj_kernels.hip is the 2 x 2 model): its
// Cholesky returns the symmetrised cotangent, so d / d Qc_inv is symmetric and d / d dt_w sees (Qc_inv + Qc_inv^T) / 2; d / d dt sees
// the matrix that Cholesky factorises, the lower triangle of W^T completed symmetrically: the upper triangle of Qc_inv on the diagonal
// blocks, all of Qc_inv^T below the diagonal (and Qc_inv above)
template <typename T>
__device__ __forceinline__ void tse2_gp_vjp(const thx_trajse2_term& tm, const SE2<T>& p1t, const SE2<T>& v1t, const SE2<T>& p2t,
                                            const SE2<T>& v2t, const T* __restrict__ ub, int b, const Eps2<T>& eps, const RecOut& out) {
  // the forward's Taylor decisions (tse2_gp, se2_log_jlog), in the run's dtype
  bool small, dsmall;
  {
    SE2<T> p1i, D;
    se2_inv(p1t, p1i);
    se2_mul(p1i, p2t, D);
    const T th = t_abs(t_atan2(D.s, D.c));
    small = th < eps.nz, dsmall = th < eps.dnz;
  }
  // pose1.local(pose2) and its two blocks, as tse2_gp forms them, in fp64
  double xi[3], Jl[9], J0[9];
  {
    SE2<double> p1i, D, Di;
    se2_inv(widen(p1t), p1i);
    se2_mul(p1i, widen(p2t), D);
    se2_log_jlog<double>(D, forced<double>(small, dsmall), xi, Jl, true);
    se2_inv(D, Di);
    double Ad[9];
    se2_adjoint(Di, Ad);
#pragma unroll
    for (int i = 0; i < 9; ++i) Ad[i] = -Ad[i];
    mat3_mul(Ad, Jl, J0);
  }
  const double dt = (double)aux_at<T>(tm, 0, b), dtw = (double)aux_at<T>(tm, 1, b);
  double up1[3], uv1[3], up2[3], uv2[3];
  load_u(ub, tm.var[0], up1), load_u(ub, tm.var[1], uv1), load_u(ub, tm.var[2], up2), load_u(ub, tm.var[3], uv2);
  const double v1[3] = {(double)v1t.x, (double)v1t.y, (double)v1t.c}, v2[3] = {(double)v2t.x, (double)v2t.y, (double)v2t.c};
  double r0[3], r1[3], rho0[3], rho1[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double c = -dt * uv1[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) c += J0[3 * i + d] * up1[d] + Jl[3 * i + d] * up2[d];
    rho0[i] = c, rho1[i] = uv2[i] - uv1[i];
    r0[i] = xi[i] - dt * v1[i], r1[i] = v2[i] - v1[i];
  }
  double Q[9], Qt[9], Qu[9], Qs[9];   // Qc_inv, its transpose, its upper triangle completed symmetrically, its symmetric part
#pragma unroll
  for (int i = 0; i < 9; ++i) Q[i] = (double)aux_at<T>(tm, 2, b, i);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Qt[3 * i + j] = Q[3 * j + i];
      Qu[3 * i + j] = i <= j ? Q[3 * i + j] : Q[3 * j + i];
      Qs[3 * i + j] = 0.5 * (Q[3 * i + j] + Q[3 * j + i]);
    }
  const double m00 = 12.0 / (dtw * dtw * dtw), m01 = -6.0 / (dtw * dtw), m11 = 4.0 / dtw;
  const double d00 = -36.0 / (dtw * dtw * dtw * dtw), d01 = 12.0 / (dtw * dtw * dtw), d11 = -4.0 / (dtw * dtw);
  out.put(0, m00 * (form3(uv1, Qu, r0) + form3(rho0, Qu, v1)) + m01 * (form3(uv1, Q, r1) + form3(rho1, Qt, v1)));
  out.put(1, -(d00 * form3(rho0, Qs, r0) + d01 * (form3(rho0, Qs, r1) + form3(rho1, Qs, r0)) + d11 * form3(rho1, Qs, r1)));
  // G = -sum_ac M_ac rho_a r_c^T; Qc_inv gets (G + G^T) / 2
  double G[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      G[3 * i + j] = -(m00 * rho0[i] * r0[j] + m01 * (rho0[i] * r1[j] + rho1[i] * r0[j]) + m11 * rho1[i] * r1[j]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out.put(2 + 3 * i + j, 0.5 * (G[3 * i + j] + G[3 * j + i]));
}

// record: 0 weight.  phi = -w^2 u_vy v_y
template <typename T>
__device__ __forceinline__ void tse2_nonholonomic_vjp(const thx_trajse2_term& tm, const SE2<T>& vel, const T* __restrict__ ub, int b,
                                                      const RecOut& out) {
  out.put(0, -2.0 * (double)aux_at<T>(tm, 0, b) * (double)ub[3 * tm.var[1] + 1] * (double)vel.y);
}

// record: 0-2 down_limit, 3-5 up_limit, 6-8 threshold, 9-11 weight.  phi = -sum_i w_i^2 sgn_i u_i err_i; the branch is tse2_hinge's,
// in T; a limit whose branch is not taken gets exactly 0 (the limits may be +-inf: nothing is multiplied by a 0 / 1 mask)
template <typename T>
__device__ __forceinline__ void tse2_hinge_vjp(const thx_trajse2_term& tm, const SE2<T>& vec, const T* __restrict__ ub, int b,
                                               const RecOut& out) {
  double w[3], uu[3], gw[3];
  tse2_weights64<T, 3>(tm, 3, b, w);
  load_u(ub, tm.var[0], uu);
  const T v[3] = {vec.x, vec.y, vec.c};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const T thr = aux_at<T>(tm, 2, b, i), lo = aux_at<T>(tm, 0, b, i), hi = aux_at<T>(tm, 1, b, i);
    const T down = lo + thr, up = hi - thr;
    const bool below = v[i] < down, above = v[i] > up;
    const double a = w[i] * w[i] * uu[i];
    double g_down = 0.0, g_up = 0.0, g_thr = 0.0;
    gw[i] = 0.0;
    if (below) g_down = a, g_thr = a, gw[i] = 2.0 * w[i] * uu[i] * (((double)lo + (double)thr) - (double)v[i]);
    if (above) g_down = 0.0, g_up = a, g_thr = -a, gw[i] = -2.0 * w[i] * uu[i] * ((double)v[i] - ((double)hi - (double)thr));
    out.put(i, g_down);
    out.put(3 + i, g_up);
    out.put(6 + i, g_thr);
  }
  out.weights(9, tm.wdim, gw);
}

// record: 0-3 target (raw x, y, cos, sin), 4-6 weight
template <typename T>
__device__ __forceinline__ void tse2_prior_se2_vjp(const thx_trajse2_term& tm, const SE2<T>& var, const T* __restrict__ ub, int b,
                                                   const Eps2<T>& eps, const RecOut& out) {
  const T* p = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  double w[3], uu[3];
  tse2_weights64<T, 3>(tm, 1, b, w);
  load_u(ub, tm.var[0], uu);
  se2_prior_vjp<T>(SE2<T>{p[0], p[1], p[2], p[3]}, var, w, uu, tm.wdim, eps, out);
}

// record: 0-2 target, 3-5 weight.  phi = -sum_i u_i w_i^2 (x_i - t_i)
template <typename T>
__device__ __forceinline__ void tse2_prior_vec_vjp(const thx_trajse2_term& tm, const SE2<T>& vec, const T* __restrict__ ub, int b,
                                                   const RecOut& out) {
  double w[3], uu[3], gw[3];
  tse2_weights64<T, 3>(tm, 1, b, w);
  load_u(ub, tm.var[0], uu);
  const double x[3] = {(double)vec.x, (double)vec.y, (double)vec.c};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    out.put(i, uu[i] * w[i] * w[i]);
    gw[i] = -2.0 * w[i] * uu[i] * (x[i] - (double)aux_at<T>(tm, 0, b, i));
  }
  out.weights(3, tm.wdim, gw);
}

// record: 0-1 target, 2-3 weight.  phi = -sum_i w_i^2 c_i (xy_i - t_i), c = R(pose) u_xy
template <typename T>
__device__ __forceinline__ void tse2_prior_xy_vjp(const thx_trajse2_term& tm, const SE2<T>& p, const T* __restrict__ ub, int b,
                                                  const RecOut& out) {
  double w[2], gw[2];
  tse2_weights64<T, 2>(tm, 1, b, w);
  const double u0 = (double)ub[3 * tm.var[0]], u1 = (double)ub[3 * tm.var[0] + 1], cs = (double)p.c, sn = (double)p.s;
  const double c[2] = {cs * u0 - sn * u1, sn * u0 + cs * u1}, xy[2] = {(double)p.x, (double)p.y};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    out.put(i, w[i] * w[i] * c[i]);
    gw[i] = -2.0 * w[i] * c[i] * (xy[i] - (double)aux_at<T>(tm, 0, b, i));
  }
  out.weights<2>(2, tm.wdim, gw);
}

// stage A: trajse2_eval_kernel's map and guards; a (term, problem) writes the entries of its kind, zeros where the term is skipped
template <typename T>
__global__ void __launch_bounds__(256)
trajse2_vjp_terms_kernel(const thx_trajse2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int V,
                         const T* __restrict__ u, int64_t ldu, int m, int64_t j_total, double* __restrict__ rec, int B, Eps2<T> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_trajse2_term& tm = terms[t];   // (read in place, as the forward does)
  const RecOut out{rec + (int64_t)t * kRec * B + b, (int64_t)B};
  bool ok = tse2_reads_ok(tm, V);
  if (ok) {
    const int dim = tse2_dim(tm.kind), nv = tse2_vars(tm.kind);
    ok = !(tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)3 * dim * nv > j_total);
  }
  if (!ok) {
    out.zeros(0, tse2_rec_count(tm.kind));
    return;
  }
  const T* ub = u + (int64_t)b * ldu;
  if (tm.kind == THX_TRAJSE2_NONHOLONOMIC) {   // (the pose is not read: its block is zero)
    tse2_nonholonomic_vjp<T>(tm, tse2_load(x, (int64_t)tm.var[1] * B + b), ub, b, out);
    return;
  }
  const SE2<T> a = tse2_load(x, (int64_t)tm.var[0] * B + b);
  switch (tm.kind) {
    case THX_TRAJSE2_COLLISION: tse2_collision_vjp<T>(tm, a, ub, b, out); return;
    case THX_TRAJSE2_HINGE: tse2_hinge_vjp<T>(tm, a, ub, b, out); return;
    case THX_TRAJSE2_PRIOR_SE2: tse2_prior_se2_vjp<T>(tm, a, ub, b, eps, out); return;
    case THX_TRAJSE2_PRIOR_VEC: tse2_prior_vec_vjp<T>(tm, a, ub, b, out); return;
    case THX_TRAJSE2_PRIOR_XY: tse2_prior_xy_vjp<T>(tm, a, ub, b, out); return;
    default: break;
  }
  const SE2<T> v1 = tse2_load(x, (int64_t)tm.var[1] * B + b);
  const SE2<T> p2 = tse2_load(x, (int64_t)tm.var[2] * B + b);
  const SE2<T> v2 = tse2_load(x, (int64_t)tm.var[3] * B + b);
  tse2_gp_vjp<T>(tm, a, v1, p2, v2, ub, b, eps, out);
}

}  // namespace thx

using namespace thx;

extern "C" int thx_trajse2_vjp(const thx_trajse2_term* terms, int32_t n_terms, const void* x, int32_t V, const void* u, int64_t ldu,
                               int32_t m, int64_t j_total, double* rec, const thx_traj2_grad_plan* plan, void* grad_out,
                               double* grid_work, int32_t B, int dtype, const thx_se2_eps* eps, void* stream) {
  const char* who = "thx_trajse2_vjp";
  // (the state is read one 4-element record per load)
  if (int rc = family_check(who, !u || !rec || !plan || !grad_out || !eps, terms, n_terms, x, 4, B, dtype,
                            V < 1 ? ": V < 1" : nullptr))
    return rc;
  if (ldu < (int64_t)3 * V) return fail(who, ": ldu < 3 V");
  if (m < 1 || j_total < 3) return fail(who, ": m < 1 or j_total < 3");
  const thx_traj2_grad_plan p = *plan;
  unsigned term_blocks = 0;
  if (int rc = family_check_vjp(who, u, rec, p, grad_out, grid_work, n_terms, B, dtype, &term_blocks)) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(trajse2_vjp_terms_kernel<float>, dim3(term_blocks), block, 0, s, terms, n_terms, (const float*)x, V,
                                  (const float*)u, ldu, m, j_total, rec, B, tse2_eps<float>(eps)),
               hipLaunchKernelGGL(trajse2_vjp_terms_kernel<double>, dim3(term_blocks), block, 0, s, terms, n_terms, (const double*)x,
                                  V, (const double*)u, ldu, m, j_total, rec, B, tse2_eps<double>(eps)));
  if (int rc = family_vjp_stage_b<thx_trajse2_term, THX_TRAJSE2_COLLISION, kRec>(rec, terms, n_terms, p, grad_out, grid_work, B, dtype, s))
    return rc;
  return check_launch(who);
}
