// Inverse kinematics on URDF chains (examples/inverse_kinematics.py of the reference): the cost family of theseus_amd/kinematics.py --
// LinkPoseCost  log(target^-1 T_link(theta)), LinkPositionCost  t_link(theta) - target, HingeCost (joint limits) and Difference
// (rest-pose prior) on Vector(dof) variables of one robot.  The torch twins are the classes of theseus_amd/kinematics.py on
// theseus_amd/se3_torch.py.
//
// thx_kin_eval: one thread per (term, problem), problems fastest.  A link term keeps O(1) state in the length of its path:
//   forward   T_link = rel_0 rel_1 ... rel_(n-1),  rel_k = origin_k * motion_k(theta)   (one pass over the path entries)
//   M         W Jlog(log(target^-1 T_link)) as three 3 x 3 blocks (pose) or W R_link (position)
//   backward  Y = (rel_(k+1) ... rel_(n-1))^-1 is carried from the last joint to the first; the body Jacobian's column of joint k is
//             Ad(Y) axis_k, and M times it goes straight to memory.  The ids of the joints on a path grow from the root to the link
//             (breadth-first numbering), so the columns between two of them -- joints that are no ancestors of the link -- are
//             zero-filled on the way and every element of the block is written once.  No per-thread array is indexed at run time.
// The rotation about a UNIT axis a is I + sin(q) [a]x + (1 - cos(q)) [a]x^2: no division, no branch.  The Taylor switches that remain
// (log, Jlog of csrc/lie.cuh) take the thresholds theseus_amd/se3_torch.py takes.
// thx_kin_error: one workgroup per problem, thread i sums the squares of terms i, i + 256, ... in fp64, then the fixed-order tree of
// term_family.cuh.
//
// The Lie chain runs in fp64 registers in either dtype (csrc/lie.cuh, "Evaluation precision": the closed forms of log / Jlog cancel
// in fp32 exactly where IK converges to, at small residual rotations); storage, the hinge and the prior are the run's dtype.
#pragma clang fp contract(off)
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

// a link term's weighted error and weighted DIM x dof block (the file's head has the scheme)
template <typename T, bool POSE>
__device__ __forceinline__ void kin_link_block(const thx_kin_term& tm, const thx_kin_joint* __restrict__ paths, const T* __restrict__ xb,
                                               int dof, int b, const Eps<double>& eps, T* __restrict__ eb, T* __restrict__ Jb) {
  constexpr int DIM = POSE ? 6 : 3;
  SE3<double> Tl;
  kin_forward<T>(tm, paths, xb, dof, Tl);
  double ev[6];
  SJac<double> M;
  kin_link_error<T, POSE>(tm, Tl, b, eps, ev, M, true);
#pragma unroll
  for (int i = 0; i < DIM; ++i) eb[i] = (T)ev[i];
  SE3<double> Y;
  kin_identity(Y);
  int next = dof;   // columns [next, dof) are written
  for (int k = tm.var[2] - 1; k >= 0; --k) {
    const thx_kin_joint& jt = paths[tm.var[1] + k];
    const bool movable = kin_movable(jt, dof);
    if (movable) {
      // the joint's twist in the link frame: Ad(Y) [0; a] = [t x (R a); R a] (revolute), Ad(Y) [a; 0] = [R a; 0] (prismatic)
      const double a0 = jt.axis[0], a1 = jt.axis[1], a2 = jt.axis[2];
      const bool rev = jt.type == THX_KIN_REVOLUTE;
      const double r0 = Y.R[0] * a0 + Y.R[1] * a1 + Y.R[2] * a2, r1 = Y.R[3] * a0 + Y.R[4] * a1 + Y.R[5] * a2,
                   r2 = Y.R[6] * a0 + Y.R[7] * a1 + Y.R[8] * a2;
      const double v0 = rev ? Y.t[1] * r2 - Y.t[2] * r1 : r0, v1 = rev ? Y.t[2] * r0 - Y.t[0] * r2 : r1,
                   v2 = rev ? Y.t[0] * r1 - Y.t[1] * r0 : r2;
      const double w0 = rev ? r0 : 0.0, w1 = rev ? r1 : 0.0, w2 = rev ? r2 : 0.0;
      const int idx = jt.theta;
      for (int c = idx + 1; c < next; ++c)
#pragma unroll
        for (int r = 0; r < DIM; ++r) Jb[(int64_t)r * dof + c] = (T)0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double top = M.a[3 * r] * v0 + M.a[3 * r + 1] * v1 + M.a[3 * r + 2] * v2;
        if (POSE) {
          top += M.c[3 * r] * w0 + M.c[3 * r + 1] * w1 + M.c[3 * r + 2] * w2;
          Jb[(int64_t)(3 + r) * dof + idx] = (T)(M.d[3 * r] * w0 + M.d[3 * r + 1] * w1 + M.d[3 * r + 2] * w2);
        }
        Jb[(int64_t)r * dof + idx] = (T)top;
      }
      next = idx < next ? idx : next;
    }
    SE3<double> rel, ri, nextY;
    kin_relative(jt, movable, movable ? (double)xb[jt.theta] : 0.0, rel);
    se3_inv(rel, ri);
    se3_mul(Y, ri, nextY);
    Y = nextY;
  }
  for (int c = 0; c < next; ++c)
#pragma unroll
    for (int r = 0; r < DIM; ++r) Jb[(int64_t)r * dof + c] = (T)0;
}

template <typename T>
__global__ void __launch_bounds__(256)
kin_eval_kernel(const thx_kin_term* __restrict__ terms, int n_terms, const thx_kin_joint* __restrict__ paths, int n_paths,
                const T* __restrict__ x, int64_t ldx, int n, int dof, T* __restrict__ J, int64_t j_total, T* __restrict__ e,
                int64_t lde, int m, int B, Eps<double> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_kin_term& tm = terms[t];   // (read in place: a private copy of the 128 bytes would live in scratch)
  if (!kin_term_ok(tm, n, dof, n_paths)) return;
  const int dim = kin_dim(tm, dof);
  if (tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)dim * dof > j_total) return;
  T* __restrict__ eb = e + (int64_t)b * lde + tm.row0;
  T* __restrict__ Jb = J + tm.j_off * B + (int64_t)dim * dof * b;
  const T* __restrict__ xb = x + (int64_t)b * ldx + tm.var[0];
  if (tm.kind == THX_KIN_HINGE || tm.kind == THX_KIN_PRIOR) {
    for (int i = 0; i < dof; ++i) {
      T err, jd;
      kin_vector_term<T>(tm, xb, b, i, err, jd);
      eb[i] = err;
      for (int k = 0; k < dof; ++k) Jb[(int64_t)i * dof + k] = i == k ? jd : (T)0;
    }
    return;
  }
  if (tm.kind == THX_KIN_POSE)
    kin_link_block<T, true>(tm, paths, xb, dof, b, eps, eb, Jb);
  else
    kin_link_block<T, false>(tm, paths, xb, dof, b, eps, eb, Jb);
}

template <typename T>
__global__ void __launch_bounds__(kErrThreads)
kin_error_kernel(const thx_kin_term* __restrict__ terms, int n_terms, const thx_kin_joint* __restrict__ paths, int n_paths,
                 const T* __restrict__ x, int64_t ldx, int n, int dof, T* __restrict__ err, int B, Eps<double> eps) {
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < n_terms; t += kErrThreads) {
    const thx_kin_term& tm = terms[t];
    if (!kin_term_ok(tm, n, dof, n_paths)) continue;
    const T* __restrict__ xb = x + (int64_t)b * ldx + tm.var[0];
    if (tm.kind == THX_KIN_HINGE || tm.kind == THX_KIN_PRIOR) {
      for (int i = 0; i < dof; ++i) {
        T ev, jd;
        kin_vector_term<T>(tm, xb, b, i, ev, jd);
        acc += (double)ev * (double)ev;
      }
    } else {
      SE3<double> Tl;
      kin_forward<T>(tm, paths, xb, dof, Tl);
      double ev[6];
      SJac<double> M;
      if (tm.kind == THX_KIN_POSE)
        kin_link_error<T, true>(tm, Tl, b, eps, ev, M, false);
      else
        kin_link_error<T, false>(tm, Tl, b, eps, ev, M, false);   // (ev[3 .. 5] = 0)
#pragma unroll
      for (int i = 0; i < 6; ++i) acc += (double)(T)ev[i] * (double)(T)ev[i];   // (the values thx_kin_eval stores)
    }
  }
  store_half_sum(acc, err + b);
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

using namespace thx;

extern "C" int thx_kin_eval(const thx_kin_term* terms, int32_t n_terms, const thx_kin_joint* paths, int32_t n_paths, const void* x,
                            int64_t ldx, int32_t n, int32_t dof, void* J, int64_t j_total, void* e, int64_t lde, int32_t m, int32_t B,
                            int dtype, const thx_lie_eps* eps, void* stream) {
  const char* who = "thx_kin_eval";
  unsigned blocks = 0;
  if (int rc = family_check(who, !J || !e || !eps || !paths, terms, n_terms, x, 1, B, dtype, kin_bad_size(paths, n_paths, ldx, n, dof)))
    return rc;
  if (int rc = family_check_eval(who, J, j_total < dof ? ": j_total < dof" : nullptr, e, lde, m, n_terms, B, dtype, &blocks)) return rc;
  const dim3 grid(blocks), block(256);
  const Eps<double> ep = kin_eps(eps, dtype);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(kin_eval_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, paths, n_paths,
                                  (const float*)x, ldx, n, dof, (float*)J, j_total, (float*)e, lde, m, B, ep),
               hipLaunchKernelGGL(kin_eval_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, paths, n_paths,
                                  (const double*)x, ldx, n, dof, (double*)J, j_total, (double*)e, lde, m, B, ep));
  return check_launch(who);
}

extern "C" int thx_kin_error(const thx_kin_term* terms, int32_t n_terms, const thx_kin_joint* paths, int32_t n_paths, const void* x,
                             int64_t ldx, int32_t n, int32_t dof, void* err, int32_t B, int dtype, const thx_lie_eps* eps,
                             void* stream) {
  const char* who = "thx_kin_error";
  if (int rc = family_check(who, !err || !eps || !paths, terms, n_terms, x, 1, B, dtype, kin_bad_size(paths, n_paths, ldx, n, dof)))
    return rc;
  if (reinterpret_cast<uintptr_t>(err) % (dtype == THX_F32 ? 4 : 8)) return fail(who, ": pointer not aligned");
  const dim3 grid((unsigned)B), block(kErrThreads);   // (B <= INT32_MAX)
  const Eps<double> ep = kin_eps(eps, dtype);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(kin_error_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, paths, n_paths,
                                  (const float*)x, ldx, n, dof, (float*)err, B, ep),
               hipLaunchKernelGGL(kin_error_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, paths, n_paths,
                                  (const double*)x, ldx, n, dof, (double*)err, B, ep));
  return check_launch(who);
}
