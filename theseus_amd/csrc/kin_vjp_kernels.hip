// The backward of the inverse-kinematics implicit step (thx_kin_vjp): with g = -sum_t J_t^T e_t what thx_kin_eval +
// thx_block_assemble form at a detached state and u a cotangent of g, the gradient of u^T g w.r.t. the auxiliary tensors -- what
// autograd computes by walking the torch classes of theseus_amd/kinematics.py and se3_torch.py back.  Per term
//   phi_t = -(J_t u) . e_t
// and no kind needs its dim x dof block for that:
//   link terms         J u = M nu with nu = J_body u = sum_k Ad(Y_k) axis_k u[theta_k], the body twist the cotangent induces at the
//                      link: six doubles accumulated on the forward's walk back from the link (kin_family.cuh), O(1) state in the
//                      length of the path; joints off the path have zero columns and never enter
//   LinkPoseCost       J u = W Jlog(xi) nu, e = W xi, xi = log(target^-1 T_link).  Weights in closed form from the values; the
//                      target through its 12 raw entries as the torch path differentiates them: se3_inv, se3_mul and se3_log_jlog
//                      of lie.cuh on Dual<double>, one pass per entry, T_link and nu held in registers.  Dual compares on its
//                      value and the values are the forward's own fp64 operations against the forward's thresholds (kin_eps), so
//                      every Taylor switch falls where the forward put it
//   LinkPositionCost   J u = W R_link nu_v, e = W (t_link - target): closed forms
//   HingeCost          closed form per component; the comparisons are kin_vector_term's, in the run's dtype; a limit whose
//                      comparison does not hold gets exactly 0 (the limits may be +-inf: nothing is multiplied by a 0 / 1 mask)
//   Difference         closed form per component
//
// Stage A (kin_vjp_terms_kernel): one thread per (term, problem), problems fastest, kin_eval_kernel's map and guards; terms are
// sorted by kind, so a wave is kind-uniform once B >= 64.  The term is read in place and a thread stores each record entry as soon
// as it has it (the stores of a wave are consecutive doubles).  The record is rec_stride >= max(18, 4 dof) doubles wide; a thread
// writes ONLY the entries its kind defines (18, 6, 4 dof, 2 dof), zeros where thx_kin_eval skips the term.
// Stage B: vjp_reduce_strided_kernel of term_family.cuh on the records.  No atomics; the family has no grids.
#pragma clang fp contract(off)
#include "kin_family.cuh"
#include "dual.cuh"

namespace thx {

using D64 = Dual<double>;
using KinRecOut = RecOutT<18>;

// the record entries a kind defines (a kind outside the four: the whole record)
__device__ __forceinline__ int kin_rec_count(int kind, int dof, int rec_stride) {
  switch (kind) {
    case THX_KIN_POSE: return 18;
    case THX_KIN_POSITION: return 6;
    case THX_KIN_HINGE: return 4 * dof;
    case THX_KIN_PRIOR: return 2 * dof;
    default: return rec_stride;
  }
}

// nu = J_body u of a link term: kin_link_block's walk with the columns contracted on the way
template <typename T>
__device__ __forceinline__ void kin_body_twist(const thx_kin_term& tm, const thx_kin_joint* __restrict__ paths, const T* __restrict__ xb,
                                               const T* __restrict__ ub, int dof, double* nu) {
#pragma unroll
  for (int i = 0; i < 6; ++i) nu[i] = 0.0;
  SE3<double> Y;
  kin_identity(Y);
  for (int k = tm.var[2] - 1; k >= 0; --k) {
    const thx_kin_joint& jt = paths[tm.var[1] + k];
    const bool movable = kin_movable(jt, dof);
    if (movable) {
      double v[3], w[3];
      kin_joint_twist(jt, Y, v, w);
      const double uk = (double)ub[jt.theta];
#pragma unroll
      for (int i = 0; i < 3; ++i) nu[i] += v[i] * uk, nu[3 + i] += w[i] * uk;
    }
    kin_step_back<T>(jt, movable, xb, Y);
  }
}

// record: 0-11 target (row major 3 x 4), 12-17 weight.  phi = -sum_i w_i^2 (Jlog nu)_i xi_i; both factors depend on the target
template <typename T>
__device__ __forceinline__ void kin_pose_vjp(const thx_kin_term& tm, const SE3<double>& Tl, const double* nu, int b,
                                             const Eps<double>& eps, const KinRecOut& out) {
  double raw[12], w[6], gw[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) raw[i] = (double)aux_at<T>(tm, 0, b, i);
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = (double)aux_at<T>(tm, 1, b, tm.wdim == 6 ? i : 0), gw[i] = 0.0;
  SE3<D64> link;
#pragma unroll
  for (int i = 0; i < 9; ++i) link.R[i] = D64(Tl.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) link.t[i] = D64(Tl.t[i]);
  const D64 nv[3] = {D64(nu[0]), D64(nu[1]), D64(nu[2])}, nw[3] = {D64(nu[3]), D64(nu[4]), D64(nu[5])};
  const Eps<D64> branch{D64(eps.nz), D64(eps.dnz), D64(eps.npi)};
#pragma unroll 1
  for (int s = 0; s < 12; ++s) {   // the unit tangent on raw entry s
    SE3<D64> target, ti, D;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) target.R[3 * i + j] = D64(raw[4 * i + j], s == 4 * i + j ? 1.0 : 0.0);
      target.t[i] = D64(raw[4 * i + 3], s == 4 * i + 3 ? 1.0 : 0.0);
    }
    se3_inv(target, ti);
    se3_mul(ti, link, D);
    D64 xi[6], Jr[9], Jt[9];
    se3_log_jlog<D64>(D, branch, xi, Jr, Jt, true);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const D64 rot = Jr[3 * i] * nw[0] + Jr[3 * i + 1] * nw[1] + Jr[3 * i + 2] * nw[2];
      const D64 top = (Jr[3 * i] * nv[0] + Jr[3 * i + 1] * nv[1] + Jr[3 * i + 2] * nv[2]
                       + (Jt[3 * i] * nw[0] + Jt[3 * i + 1] * nw[1] + Jt[3 * i + 2] * nw[2])) * xi[i];
      const D64 bot = rot * xi[3 + i];
      acc += w[i] * w[i] * top.d + w[3 + i] * w[3 + i] * bot.d;
      gw[i] = -2.0 * w[i] * top.v, gw[3 + i] = -2.0 * w[3 + i] * bot.v;
    }
    out.put(s, -acc);
  }
  out.weights<6>(12, tm.wdim, gw);
}

// record: 0-2 target, 3-5 weight.  phi = -sum_i w_i^2 (R_link nu_v)_i (t_link - target)_i
template <typename T>
__device__ __forceinline__ void kin_position_vjp(const thx_kin_term& tm, const SE3<double>& Tl, const double* nu, int b,
                                                 const KinRecOut& out) {
  double c[3], gw[3];
  mat3_vec(Tl.R, nu, c);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double w = (double)aux_at<T>(tm, 1, b, tm.wdim == 3 ? i : 0);
    out.put(i, w * w * c[i]);
    gw[i] = -2.0 * w * c[i] * (Tl.t[i] - (double)aux_at<T>(tm, 0, b, i));
  }
  out.weights<3>(3, tm.wdim, gw);
}

// record: 0... down_limit, dof... up_limit, 2 dof... threshold, 3 dof... weight (hinge);  0... target, dof... weight (prior).
// phi = -sum_i jd_i u_i err_i with kin_vector_term's jd and err; the hinge's branch is decided as there, in T
template <typename T>
__device__ __forceinline__ void kin_vector_vjp(const thx_kin_term& tm, const T* __restrict__ xb, const T* __restrict__ ub, int dof,
                                               int b, const KinRecOut& out) {
  const bool hinge = tm.kind == THX_KIN_HINGE;
  const int wbase = hinge ? 3 * dof : dof;
  double sum = 0.0;
  for (int i = 0; i < dof; ++i) {
    const T v = xb[i];
    const double uu = (double)ub[i];
    double gw = 0.0;
    if (hinge) {
      const double w = (double)aux_at<T>(tm, 3, b, tm.wdim == 1 ? 0 : i);
      const T thr = aux_at<T>(tm, 2, b, i), lo = aux_at<T>(tm, 0, b, i), hi = aux_at<T>(tm, 1, b, i);
      const T down = lo + thr, up = hi - thr;
      const bool below = v < down, above = v > up;
      const double a = w * w * uu;
      double g_down = 0.0, g_up = 0.0, g_thr = 0.0;
      if (below) g_down = a, g_thr = a, gw = 2.0 * w * uu * (((double)lo + (double)thr) - (double)v);
      if (above) g_down = 0.0, g_up = a, g_thr = -a, gw = -2.0 * w * uu * ((double)v - ((double)hi - (double)thr));
      out.put(i, g_down);
      out.put(dof + i, g_up);
      out.put(2 * dof + i, g_thr);
    } else {
      const double w = (double)aux_at<T>(tm, 1, b, tm.wdim == 1 ? 0 : i);
      out.put(i, w * w * uu);
      gw = -2.0 * w * uu * ((double)v - (double)aux_at<T>(tm, 0, b, i));
    }
    // a DiagonalCostWeight gets the per-row values, a ScaleCostWeight their sum (in index order) and zeros behind it
    sum += gw;
    if (tm.wdim != 1 || i > 0) out.put(wbase + i, tm.wdim != 1 ? gw : 0.0);
  }
  if (tm.wdim == 1) out.put(wbase, sum);
}

// stage A: kin_eval_kernel's map and guards; a (term, problem) writes the entries of its kind, zeros where the term is skipped
template <typename T>
__global__ void __launch_bounds__(256)
kin_vjp_terms_kernel(const thx_kin_term* __restrict__ terms, int n_terms, const thx_kin_joint* __restrict__ paths, int n_paths,
                     const T* __restrict__ x, int64_t ldx, int n, int dof, const T* __restrict__ u, int64_t ldu, int m, int64_t j_total,
                     double* __restrict__ rec, int rec_stride, int B, Eps<double> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_kin_term& tm = terms[t];   // (read in place, as the forward does)
  const KinRecOut out{rec + (int64_t)t * rec_stride * B + b, (int64_t)B};
  bool ok = kin_term_ok(tm, n, dof, n_paths);
  if (ok) {
    const int dim = kin_dim(tm, dof);
    ok = !(tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)dim * dof > j_total);
  }
  if (!ok) {
    out.zeros(0, kin_rec_count(tm.kind, dof, rec_stride));
    return;
  }
  const T* __restrict__ xb = x + (int64_t)b * ldx + tm.var[0];
  const T* __restrict__ ub = u + (int64_t)b * ldu + tm.var[0];
  if (tm.kind == THX_KIN_HINGE || tm.kind == THX_KIN_PRIOR) {
    kin_vector_vjp<T>(tm, xb, ub, dof, b, out);
    return;
  }
  SE3<double> Tl;
  kin_forward<T>(tm, paths, xb, dof, Tl);
  double nu[6];
  kin_body_twist<T>(tm, paths, xb, ub, dof, nu);
  if (tm.kind == THX_KIN_POSE)
    kin_pose_vjp<T>(tm, Tl, nu, b, eps, out);
  else
    kin_position_vjp<T>(tm, Tl, nu, b, out);
}

}  // namespace thx

using namespace thx;

extern "C" int thx_kin_vjp(const thx_kin_term* terms, int32_t n_terms, const thx_kin_joint* paths, int32_t n_paths, const void* x,
                           int64_t ldx, int32_t n, int32_t dof, const void* u, int64_t ldu, int32_t m, int64_t j_total, double* rec,
                           int32_t rec_stride, const thx_traj2_grad_plan* plan, void* grad_out, int32_t B, int dtype,
                           const thx_lie_eps* eps, void* stream) {
  const char* who = "thx_kin_vjp";
  if (int rc = family_check(who, !u || !rec || !plan || !grad_out || !eps || !paths, terms, n_terms, x, 1, B, dtype,
                            kin_bad_size(paths, n_paths, ldx, n, dof)))
    return rc;
  if (ldu < n) return fail(who, ": ldu < n");
  if (m < 1 || j_total < dof) return fail(who, ": m < 1 or j_total < dof");
  if (rec_stride < 18 || (int64_t)rec_stride < (int64_t)4 * dof) return fail(who, ": rec_stride < max(18, 4 dof)");
  const thx_traj2_grad_plan p = *plan;
  if (p.n_grids > 0) return fail(who, ": the family has no grids (n_grids != 0)");
  unsigned term_blocks = 0;
  if (int rc = family_check_vjp(who, u, rec, p, grad_out, nullptr, n_terms, B, dtype, &term_blocks)) return rc;
  hipStream_t s = as_stream(stream);
  const dim3 block(256);
  const Eps<double> ep = kin_eps(eps, dtype);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(kin_vjp_terms_kernel<float>, dim3(term_blocks), block, 0, s, terms, n_terms, paths, n_paths,
                                  (const float*)x, ldx, n, dof, (const float*)u, ldu, m, j_total, rec, rec_stride, B, ep),
               hipLaunchKernelGGL(kin_vjp_terms_kernel<double>, dim3(term_blocks), block, 0, s, terms, n_terms, paths, n_paths,
                                  (const double*)x, ldx, n, dof, (const double*)u, ldu, m, j_total, rec, rec_stride, B, ep));
  if (p.n_tensors > 0) {
    const dim3 grid((unsigned)((int64_t)p.n_tensors * B));
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL(vjp_reduce_strided_kernel<float>, grid, block, 0, s, rec, rec_stride, n_terms, p.tensors, p.pairs,
                                    p.n_pairs, (float*)grad_out, p.out_elems, B),
                 hipLaunchKernelGGL(vjp_reduce_strided_kernel<double>, grid, block, 0, s, rec, rec_stride, n_terms, p.tensors, p.pairs,
                                    p.n_pairs, (double*)grad_out, p.out_elems, B));
  }
  return check_launch(who);
}
