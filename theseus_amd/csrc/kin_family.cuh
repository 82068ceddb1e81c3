// What the forward (kin_kernels.hip: thx_kin_eval, thx_kin_error) and the backward of the implicit step (kin_vjp_kernels.hip:
// thx_kin_vjp) of the inverse-kinematics family share: the guards of a term, the forward kinematics along a path, the weighted error
// of a link term, the hinge / prior component, and the two pieces of the walk from the link back to the root -- the twist of a joint
// in the link frame and the step Y <- Y rel^-1.  Included after the source's own ``#pragma clang fp contract(off)``.
#pragma once
#include "term_family.cuh"
#include "lie.cuh"

namespace thx {

__device__ __forceinline__ void kin_identity(SE3<double>& X) {
#pragma unroll
  for (int i = 0; i < 9; ++i) X.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  X.t[0] = X.t[1] = X.t[2] = 0.0;
}

// a joint that moves, with a column inside the block
__device__ __forceinline__ bool kin_movable(const thx_kin_joint& jt, int dof) {
  return (jt.type == THX_KIN_REVOLUTE || jt.type == THX_KIN_PRISMATIC) && jt.theta >= 0 && jt.theta < dof;
}

// rel = origin * motion(q)
__device__ __forceinline__ void kin_relative(const thx_kin_joint& jt, bool movable, double q, SE3<double>& rel) {
  double O[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    O[3 * i] = jt.origin[4 * i];
    O[3 * i + 1] = jt.origin[4 * i + 1];
    O[3 * i + 2] = jt.origin[4 * i + 2];
    rel.t[i] = jt.origin[4 * i + 3];
  }
  const double a[3] = {jt.axis[0], jt.axis[1], jt.axis[2]};
  if (movable && jt.type == THX_KIN_REVOLUTE) {
    const double s = sin(q), c1 = 1.0 - cos(q);
    const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
    double K2[9], Rq[9];
    mat3_mul(K, K, K2);
#pragma unroll
    for (int i = 0; i < 9; ++i) Rq[i] = ((i % 4 == 0) ? 1.0 : 0.0) + s * K[i] + c1 * K2[i];
    mat3_mul(O, Rq, rel.R);
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) rel.R[i] = O[i];
    if (movable) {   // prismatic
      const double qa[3] = {q * a[0], q * a[1], q * a[2]};
      double d[3];
      mat3_vec(O, qa, d);
      rel.t[0] = d[0] + rel.t[0];
      rel.t[1] = d[1] + rel.t[1];
      rel.t[2] = d[2] + rel.t[2];
    }
  }
}

// the term's sizes fit the buffers; -> its rows
__device__ __forceinline__ int kin_dim(const thx_kin_term& tm, int dof) {
  return tm.kind == THX_KIN_POSE ? 6 : (tm.kind == THX_KIN_POSITION ? 3 : dof);
}
__device__ __forceinline__ bool kin_term_ok(const thx_kin_term& tm, int n, int dof, int n_paths) {
  if (tm.kind < THX_KIN_POSE || tm.kind > THX_KIN_PRIOR || tm.var[0] < 0 || tm.var[0] + dof > n) return false;
  if (tm.kind == THX_KIN_POSE) {
    if (tm.wdim != 1 && tm.wdim != 6) return false;
  } else if (tm.kind == THX_KIN_POSITION) {
    if (tm.wdim != 1 && tm.wdim != 3) return false;
  } else {
    return tm.wdim == 1 || tm.wdim == dof;
  }
  return tm.var[1] >= 0 && tm.var[2] >= 0 && tm.var[2] <= THX_KIN_MAX_PATH && (int64_t)tm.var[1] + tm.var[2] <= (int64_t)n_paths;
}

// T_link of a link term
template <typename T>
__device__ __forceinline__ void kin_forward(const thx_kin_term& tm, const thx_kin_joint* __restrict__ paths, const T* __restrict__ xb,
                                            int dof, SE3<double>& Tl) {
  kin_identity(Tl);
  for (int k = 0; k < tm.var[2]; ++k) {
    const thx_kin_joint& jt = paths[tm.var[1] + k];
    const bool movable = kin_movable(jt, dof);
    SE3<double> rel, next;
    kin_relative(jt, movable, movable ? (double)xb[jt.theta] : 0.0, rel);
    se3_mul(Tl, rel, next);
    Tl = next;
  }
}

// the weighted error of a link term (6 or 3 values in ev) and, want_jac, M: pose  a = W_v Jr, c = W_v Jt, d = W_w Jr;
// position  a = W R_link
template <typename T, bool POSE>
__device__ __forceinline__ void kin_link_error(const thx_kin_term& tm, const SE3<double>& Tl, int b, const Eps<double>& eps, double* ev,
                                               SJac<double>& M, bool want_jac) {
  if (POSE) {
    SE3<double> target;
    double w[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      target.R[3 * i] = (double)aux_at<T>(tm, 0, b, 4 * i);
      target.R[3 * i + 1] = (double)aux_at<T>(tm, 0, b, 4 * i + 1);
      target.R[3 * i + 2] = (double)aux_at<T>(tm, 0, b, 4 * i + 2);
      target.t[i] = (double)aux_at<T>(tm, 0, b, 4 * i + 3);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = (double)aux_at<T>(tm, 1, b, tm.wdim == 6 ? i : 0);
    local_eval<double>(target, Tl, w, eps, ev, &M, want_jac);
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double w = (double)aux_at<T>(tm, 1, b, tm.wdim == 3 ? i : 0);
      ev[i] = (Tl.t[i] - (double)aux_at<T>(tm, 0, b, i)) * w;
      ev[3 + i] = 0.0;
      M.a[3 * i] = Tl.R[3 * i] * w;
      M.a[3 * i + 1] = Tl.R[3 * i + 1] * w;
      M.a[3 * i + 2] = Tl.R[3 * i + 2] * w;
    }
  }
}

// HingeCost / Difference, component i: the weighted error and the weighted diagonal entry of the Jacobian
template <typename T>
__device__ __forceinline__ void kin_vector_term(const thx_kin_term& tm, const T* __restrict__ xb, int b, int i, T& err, T& jd) {
  const T v = xb[i];
  if (tm.kind == THX_KIN_HINGE) {
    const T w = aux_at<T>(tm, 3, b, tm.wdim == 1 ? 0 : i), thr = aux_at<T>(tm, 2, b, i);
    const T down = aux_at<T>(tm, 0, b, i) + thr, up = aux_at<T>(tm, 1, b, i) - thr;
    const bool below = v < down, above = v > up;
    T r = below ? down - v : (T)0;
    r = above ? v - up : r;
    err = r * w;
    jd = (above ? (T)1 : (below ? (T)-1 : (T)0)) * w;
  } else {
    const T w = aux_at<T>(tm, 1, b, tm.wdim == 1 ? 0 : i);
    err = (v - aux_at<T>(tm, 0, b, i)) * w;
    jd = w;
  }
}

// The walk from the link back to the root carries Y = (rel_(k+1) ... rel_(n-1))^-1 (kin_link_block of kin_kernels.hip spells these
// two steps out: with the calls the compiler orders its branches differently).  The twist of movable joint k in the link frame,
// the body Jacobian's column: Ad(Y) [0; a] = [t x (R a); R a] (revolute), Ad(Y) [a; 0] = [R a; 0] (prismatic)
__device__ __forceinline__ void kin_joint_twist(const thx_kin_joint& jt, const SE3<double>& Y, double* v, double* w) {
  const double a0 = jt.axis[0], a1 = jt.axis[1], a2 = jt.axis[2];
  const bool rev = jt.type == THX_KIN_REVOLUTE;
  const double r0 = Y.R[0] * a0 + Y.R[1] * a1 + Y.R[2] * a2, r1 = Y.R[3] * a0 + Y.R[4] * a1 + Y.R[5] * a2,
               r2 = Y.R[6] * a0 + Y.R[7] * a1 + Y.R[8] * a2;
  v[0] = rev ? Y.t[1] * r2 - Y.t[2] * r1 : r0, v[1] = rev ? Y.t[2] * r0 - Y.t[0] * r2 : r1, v[2] = rev ? Y.t[0] * r1 - Y.t[1] * r0 : r2;
  w[0] = rev ? r0 : 0.0, w[1] = rev ? r1 : 0.0, w[2] = rev ? r2 : 0.0;
}
// ... and its step past joint k: Y <- Y rel_k^-1
template <typename T>
__device__ __forceinline__ void kin_step_back(const thx_kin_joint& jt, bool movable, const T* __restrict__ xb, SE3<double>& Y) {
  SE3<double> rel, ri, nextY;
  kin_relative(jt, movable, movable ? (double)xb[jt.theta] : 0.0, rel);
  se3_inv(rel, ri);
  se3_mul(Y, ri, nextY);
  Y = nextY;
}

// the family's own size checks: the message of the first that fails
inline const char* kin_bad_size(const void* paths, int32_t n_paths, int64_t ldx, int32_t n, int32_t dof) {
  if (n_paths < 0) return ": n_paths < 0";
  if (dof < 1) return ": dof < 1";
  if (n < dof) return ": n < dof";
  if (ldx < n) return ": ldx < n";
  if (reinterpret_cast<uintptr_t>(paths) % 8) return ": pointer not aligned";
  return nullptr;
}

// the thresholds a run of ``dtype`` compares against, as the fp64 registers see them
inline Eps<double> kin_eps(const thx_lie_eps* e, int dtype) {
  if (dtype == THX_F32) return Eps<double>{(double)(float)e->near_zero, (double)(float)e->d_near_zero, (double)(float)e->near_pi};
  return make_eps<double>(e);
}

}  // namespace thx
