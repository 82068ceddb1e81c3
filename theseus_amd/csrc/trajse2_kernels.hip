// SE2 motion planning (examples/se2_planning.py of the reference: MotionPlanner with pose_type=SE2, nonholonomic_w, positive_vel_w):
// the cost family of the planner's objective -- Collision2D at xy(pose) (theseus/embodied/collision/collision.py:44-73 over
// SignedDistanceField2D.signed_distance), GPMotionModel on (SE2, Vector, SE2, Vector) with GPCostWeight (theseus/embodied/
// motionmodel/double_integrator.py:48-80, 131-170), Nonholonomic on SE2 and HingeCost (motionmodel/misc.py), Difference priors on SE2
// and on 3-vectors (theseus/embodied/misc/local_cost_fn.py:16-75) and the planner's xy goal cost (motion_planner.py:15-54) --
// evaluated by ONE launch instead of one torch call chain per cost object.
//
// The state is (V, B, 4), one 4-element record per optimisation variable and problem: an SE2 pose [x, y, cos, sin] or a velocity
// [v0, v1, v2, pad]; a record is ONE vector load, the pad element is written 0 by the host and by thx_trajse2_retract and its value is
// never used.
// thx_trajse2_eval: one thread per (term, problem), problems fastest; the host sorts the terms by kind, so a wave takes one branch
// except where two kinds meet.  A thread writes the WEIGHTED Jacobian blocks and the weighted error where thx_block_assemble's term
// tables point (thx_push2_eval's layout: every block is dim x 3).
// thx_trajse2_error: one workgroup per problem; thread i sums the squares of terms i, i + 256, ... in fp64, then a fixed-order tree.
// thx_trajse2_retract: one thread per (variable, problem); SE2 records as thx_se2_retract (exp and product in fp64), velocity records
// x + step * delta.
//
// Everything runs in the run's dtype with contraction off (the pragma below covers the SE2 helpers included after it) and in the
// reference's operation order wherever a branch is decided (grid bounds, floor, d > eps, the hinge comparisons, Taylor switches,
// atan2 arguments), so a kink lands where the torch classes of theseus_amd/embodied.py put it.  Registers only; LDS: the reduction
// of thx_trajse2_error.
#pragma clang fp contract(off)
#include "term_family.cuh"
#include "lie_se2.cuh"

namespace thx {

// one state record as ONE vector load (the record is 4 * sizeof(T) aligned: checked on the host)
__device__ __forceinline__ SE2<float> tse2_load(const float* __restrict__ x, int64_t rec) {
  const float4 v = reinterpret_cast<const float4*>(x)[rec];
  return SE2<float>{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ SE2<double> tse2_load(const double* __restrict__ x, int64_t rec) {
  const double4 v = reinterpret_cast<const double4*>(x)[rec];
  return SE2<double>{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void tse2_store(float* __restrict__ x, int64_t rec, float a, float b, float c, float d) {
  reinterpret_cast<float4*>(x)[rec] = make_float4(a, b, c, d);
}
__device__ __forceinline__ void tse2_store(double* __restrict__ x, int64_t rec, double a, double b, double c, double d) {
  reinterpret_cast<double4*>(x)[rec] = make_double4(a, b, c, d);
}

// the row weights of a Scale (wdim 1) / DiagonalCostWeight (wdim = n) at aux slot k
template <typename T, int n>
__device__ __forceinline__ void tse2_weights(const thx_trajse2_term& tm, int k, int b, T* w) {
  w[0] = aux_at<T>(tm, k, b, 0);
#pragma unroll
  for (int i = 1; i < n; ++i) w[i] = tm.wdim == n ? aux_at<T>(tm, k, b, i) : w[0];
}

// Collision2D at the pose's translation: weighted error (1) and the weighted 1 x 3 block  -(dd/dxy) [R, 0]
template <typename T>
__device__ __forceinline__ T tse2_collision(const thx_trajse2_term& tm, const SE2<T>& p, int b, T* __restrict__ J) {
  const T* sdf = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T eps = aux_at<T>(tm, 3, b), w = aux_at<T>(tm, 4, b);
  T dist, j1, j2;
  sdf_bilinear<T>(sdf, tm.rows, tm.cols, aux_at<T>(tm, 1, b, 0), aux_at<T>(tm, 1, b, 1), aux_at<T>(tm, 2, b), p.x, p.y, dist, j1, j2);
  T err = eps - dist;                         // collision.py:61-62
  if (err < (T)0) err = (T)0;
  if (J) {
    // :56-58 jac (1 x 2) @ Jxy (se2.py: [[c, -s, 0], [s, c, 0]]), then :71-73
    T g0 = j1 * p.c + j2 * p.s, g1 = j1 * -p.s + j2 * p.c;
    if (dist > eps) g0 = (T)0, g1 = (T)0;
    J[0] = -g0 * w;
    J[1] = -g1 * w;
    J[2] = (T)0;
  }
  return err * w;
}

// y = Lq^T x for the upper-triangular Lq^T = [[t0, t1, t2], [0, t3, t4], [0, 0, t5]]
template <typename T>
__device__ __forceinline__ void tse2_upper(const T* t, T x0, T x1, T x2, T& y0, T& y1, T& y2) {
  y0 = t[0] * x0 + t[1] * x1 + t[2] * x2;
  y1 = t[3] * x1 + t[4] * x2;
  y2 = t[5] * x2;
}

// GPMotionModel: weighted error (6) and the four weighted 6 x 3 blocks (pose1, vel1, pose2, vel2), block s at J + s * jstep.
// U = chol(W^T)^T, W = M (x) Qc_inv (double_integrator.py:131-152) = chol(M)^T (x) chol(Qc_inv^T)^T
//   = [[a Lq^T, bb Lq^T], [0, c Lq^T]]: applied by halves, U [x0; x1] = [Lq^T (a x0 + bb x1); Lq^T (c x1)].
template <typename T>
__device__ __forceinline__ void tse2_gp(const thx_trajse2_term& tm, const SE2<T>& p1, const SE2<T>& v1, const SE2<T>& p2,
                                        const SE2<T>& v2, int b, const Eps2<T>& eps, T* __restrict__ e, T* __restrict__ J,
                                        int64_t jstep) {
  const T dt = aux_at<T>(tm, 0, b), dtw = aux_at<T>(tm, 1, b);
  // (the reference factorises W^T: of a Qc_inv that is not exactly symmetric it reads the UPPER triangle)
  const T q00 = aux_at<T>(tm, 2, b, 0), q01 = aux_at<T>(tm, 2, b, 1), q02 = aux_at<T>(tm, 2, b, 2);
  const T q11 = aux_at<T>(tm, 2, b, 4), q12 = aux_at<T>(tm, 2, b, 5), q22 = aux_at<T>(tm, 2, b, 8);
  const T m11 = (T)12 / (dtw * dtw * dtw), m21 = (T)-6 / (dtw * dtw), m22 = (T)4 / dtw;
  const T a = t_sqrt(m11), bb = m21 / a, c = t_sqrt(m22 - bb * bb);
  T t[6];   // Lq^T, row major upper triangle
  t[0] = t_sqrt(q00);
  t[1] = q01 / t[0];
  t[2] = q02 / t[0];
  t[3] = t_sqrt(q11 - t[1] * t[1]);
  t[4] = (q12 - t[2] * t[1]) / t[3];
  t[5] = t_sqrt(q22 - t[2] * t[2] - t[4] * t[4]);
  // pose1.local(pose2) (lie_group.py:180-195)
  SE2<T> p1i, D;
  se2_inv(p1, p1i);
  se2_mul(p1i, p2, D);
  T xi[3], Jl[9];
  se2_log_jlog(D, eps, xi, Jl, J != nullptr);
  const T r0[3] = {xi[0] - dt * v1.x, xi[1] - dt * v1.y, xi[2] - dt * v1.c};   // double_integrator.py:53-56
  const T r1[3] = {v2.x - v1.x, v2.y - v1.y, v2.c - v1.c};
  tse2_upper(t, a * r0[0] + bb * r1[0], a * r0[1] + bb * r1[1], a * r0[2] + bb * r1[2], e[0], e[1], e[2]);
  tse2_upper(t, c * r1[0], c * r1[1], c * r1[2], e[3], e[4], e[5]);
  if (!J) return;
  // d local / d pose1 = -Ad(D^-1) Jlog, d local / d pose2 = Jlog
  SE2<T> Di;
  se2_inv(D, Di);
  T Ad[9], J0[9];
  se2_adjoint(Di, Ad);
#pragma unroll
  for (int i = 0; i < 9; ++i) Ad[i] = -Ad[i];
  mat3_mul(Ad, Jl, J0);
  T* P1 = J;
  T* V1 = J + jstep;
  T* P2 = J + 2 * jstep;
  T* V2 = J + 3 * jstep;
  const T top = -dt * a - bb;   // vel1: U [-dt I; -I]
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    T y0, y1, y2;
    tse2_upper(t, a * J0[d], a * J0[3 + d], a * J0[6 + d], y0, y1, y2);
    P1[d] = y0, P1[3 + d] = y1, P1[6 + d] = y2;
    tse2_upper(t, a * Jl[d], a * Jl[3 + d], a * Jl[6 + d], y0, y1, y2);
    P2[d] = y0, P2[3 + d] = y1, P2[6 + d] = y2;
    // column d of Lq^T itself: rows 0 .. 2
    const T c0 = d == 0 ? t[0] : (d == 1 ? t[1] : t[2]);
    const T c1 = d == 0 ? (T)0 : (d == 1 ? t[3] : t[4]);
    const T c2 = d == 2 ? t[5] : (T)0;
    V1[d] = top * c0, V1[3 + d] = top * c1, V1[6 + d] = top * c2;
    V1[9 + d] = -c * c0, V1[12 + d] = -c * c1, V1[15 + d] = -c * c2;
    V2[d] = bb * c0, V2[3 + d] = bb * c1, V2[6 + d] = bb * c2;
    V2[9 + d] = c * c0, V2[12 + d] = c * c1, V2[15 + d] = c * c2;
    P1[9 + d] = P1[12 + d] = P1[15 + d] = (T)0;
    P2[9 + d] = P2[12 + d] = P2[15 + d] = (T)0;
  }
}

// Nonholonomic on SE2: the body-frame sideways velocity; blocks (pose: 0, vel: [0, w, 0])
template <typename T>
__device__ __forceinline__ T tse2_nonholonomic(const thx_trajse2_term& tm, const SE2<T>& vel, int b, T* __restrict__ J, int64_t jstep) {
  const T w = aux_at<T>(tm, 0, b);
  if (J) {
    J[0] = J[1] = J[2] = (T)0;
    J[jstep] = (T)0, J[jstep + 1] = w, J[jstep + 2] = (T)0;
  }
  return vel.y * w;
}

// HingeCost (misc.py:62-84): strict comparisons, "above" overrides "below", selected by branches (the limits may be +-inf:
// (v - inf) * 0 is NaN)
template <typename T>
__device__ __forceinline__ void tse2_hinge(const thx_trajse2_term& tm, const SE2<T>& vec, int b, T* __restrict__ e, T* __restrict__ J) {
  T w[3];
  tse2_weights<T, 3>(tm, 3, b, w);
  const T v[3] = {vec.x, vec.y, vec.c};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const T thr = aux_at<T>(tm, 2, b, i);
    const T down = aux_at<T>(tm, 0, b, i) + thr, up = aux_at<T>(tm, 1, b, i) - thr;
    const bool below = v[i] < down, above = v[i] > up;
    T err = (T)0, sgn = (T)0;
    if (below) err = down - v[i], sgn = (T)-1;
    if (above) err = v[i] - up, sgn = (T)1;
    e[i] = err * w[i];
    if (J) {
#pragma unroll
      for (int d = 0; d < 3; ++d) J[3 * i + d] = d == i ? sgn * w[i] : (T)0;
    }
  }
}

template <typename T>
__device__ __forceinline__ void tse2_prior_se2(const thx_trajse2_term& tm, const SE2<T>& var, int b, const Eps2<T>& eps,
                                               T* __restrict__ e, T* __restrict__ J) {
  const T* p = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const SE2<T> target{p[0], p[1], p[2], p[3]};
  T w[3], Jl[9];
  tse2_weights<T, 3>(tm, 1, b, w);
  local_eval2(target, var, w, eps, e, Jl, J != nullptr);
  if (J) {
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = Jl[i];
  }
}

// Difference on a 3-vector: e = (x - target) * w, J = diag(w)
template <typename T>
__device__ __forceinline__ void tse2_prior_vec(const thx_trajse2_term& tm, const SE2<T>& vec, int b, T* __restrict__ e,
                                               T* __restrict__ J) {
  T w[3];
  tse2_weights<T, 3>(tm, 1, b, w);
  e[0] = (vec.x - aux_at<T>(tm, 0, b, 0)) * w[0];
  e[1] = (vec.y - aux_at<T>(tm, 0, b, 1)) * w[1];
  e[2] = (vec.c - aux_at<T>(tm, 0, b, 2)) * w[2];
  if (J) {
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0) ? w[i / 4] : (T)0;
  }
}

// the planner's goal cost: e = (xy(pose) - target) * w, J = diag(w) [R, 0]
template <typename T>
__device__ __forceinline__ void tse2_prior_xy(const thx_trajse2_term& tm, const SE2<T>& p, int b, T* __restrict__ e, T* __restrict__ J) {
  T w[2];
  tse2_weights<T, 2>(tm, 1, b, w);
  e[0] = (p.x - aux_at<T>(tm, 0, b, 0)) * w[0];
  e[1] = (p.y - aux_at<T>(tm, 0, b, 1)) * w[1];
  if (J) {
    J[0] = p.c * w[0], J[1] = -p.s * w[0], J[2] = (T)0;
    J[3] = p.s * w[1], J[4] = p.c * w[1], J[5] = (T)0;
  }
}

__device__ __forceinline__ int tse2_dim(int kind) {
  return kind == THX_TRAJSE2_GP ? 6
         : (kind == THX_TRAJSE2_COLLISION || kind == THX_TRAJSE2_NONHOLONOMIC) ? 1
         : (kind == THX_TRAJSE2_PRIOR_XY ? 2 : 3);
}
__device__ __forceinline__ int tse2_vars(int kind) {
  return kind == THX_TRAJSE2_GP ? 4 : (kind == THX_TRAJSE2_NONHOLONOMIC ? 2 : 1);
}

// the kind is one of the seven, every record a term reads lies inside the state, a weight is as wide as 1 or as the cost
__device__ __forceinline__ bool tse2_reads_ok(const thx_trajse2_term& tm, int V) {
  if (tm.kind < THX_TRAJSE2_COLLISION || tm.kind > THX_TRAJSE2_PRIOR_XY) return false;
  const int nv = tse2_vars(tm.kind);
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < nv && (tm.var[s] < 0 || tm.var[s] >= V)) return false;
  if (tm.kind == THX_TRAJSE2_COLLISION) return tm.rows >= 1 && tm.cols >= 1;
  if (tm.kind == THX_TRAJSE2_GP || tm.kind == THX_TRAJSE2_NONHOLONOMIC) return true;
  return tm.wdim == 1 || tm.wdim == tse2_dim(tm.kind);
}

// weighted error of term tm for problem b into ev (dim values); Jb != nullptr: also the weighted blocks, block s at Jb + s * jstep
template <typename T>
__device__ __forceinline__ void tse2_term(const thx_trajse2_term& tm, const T* __restrict__ x, int B, int b, const Eps2<T>& eps,
                                          T* __restrict__ ev, T* __restrict__ Jb, int64_t jstep) {
  if (tm.kind == THX_TRAJSE2_NONHOLONOMIC) {   // (the pose is not read: its block is zero)
    ev[0] = tse2_nonholonomic<T>(tm, tse2_load(x, (int64_t)tm.var[1] * B + b), b, Jb, jstep);
    return;
  }
  const SE2<T> a = tse2_load(x, (int64_t)tm.var[0] * B + b);
  switch (tm.kind) {
    case THX_TRAJSE2_COLLISION: ev[0] = tse2_collision<T>(tm, a, b, Jb); return;
    case THX_TRAJSE2_HINGE: tse2_hinge<T>(tm, a, b, ev, Jb); return;
    case THX_TRAJSE2_PRIOR_SE2: tse2_prior_se2<T>(tm, a, b, eps, ev, Jb); return;
    case THX_TRAJSE2_PRIOR_VEC: tse2_prior_vec<T>(tm, a, b, ev, Jb); return;
    case THX_TRAJSE2_PRIOR_XY: tse2_prior_xy<T>(tm, a, b, ev, Jb); return;
    default: break;
  }
  const SE2<T> v1 = tse2_load(x, (int64_t)tm.var[1] * B + b);
  const SE2<T> p2 = tse2_load(x, (int64_t)tm.var[2] * B + b);
  const SE2<T> v2 = tse2_load(x, (int64_t)tm.var[3] * B + b);
  tse2_gp<T>(tm, a, v1, p2, v2, b, eps, ev, Jb, jstep);
}

template <typename T>
__global__ void __launch_bounds__(256)
trajse2_eval_kernel(const thx_trajse2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int V, T* __restrict__ J,
                    int64_t j_total, T* __restrict__ e, int64_t lde, int m, int B, Eps2<T> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_trajse2_term& tm = terms[t];   // (read in place: a private copy of the 128 bytes would live in scratch)
  if (!tse2_reads_ok(tm, V)) return;
  const int dim = tse2_dim(tm.kind), nv = tse2_vars(tm.kind);
  if (tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)3 * dim * nv > j_total) return;
  T* eb = e + (int64_t)b * lde + tm.row0;
  T* Jb = J + tm.j_off * B + (int64_t)3 * dim * b;
  T ev[6];
  tse2_term<T>(tm, x, B, b, eps, ev, Jb, (int64_t)3 * dim * B);
  eb[0] = ev[0];
  if (dim >= 2) eb[1] = ev[1];
  if (dim >= 3) eb[2] = ev[2];
  if (dim == 6) eb[3] = ev[3], eb[4] = ev[4], eb[5] = ev[5];
}

template <typename T>
__global__ void __launch_bounds__(kErrThreads)
trajse2_error_kernel(const thx_trajse2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int V, T* __restrict__ err,
                     int B, Eps2<T> eps) {
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < n_terms; t += kErrThreads) {
    const thx_trajse2_term& tm = terms[t];   // (read in place: a private copy of the 128 bytes would live in scratch)
    if (!tse2_reads_ok(tm, V)) continue;
    T ev[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    tse2_term<T>(tm, x, B, b, eps, ev, nullptr, 0);
    const int dim = tse2_dim(tm.kind);
    acc += (double)ev[0] * (double)ev[0];
    if (dim >= 2) acc += (double)ev[1] * (double)ev[1];
    if (dim >= 3) acc += (double)ev[2] * (double)ev[2];
    if (dim == 6) acc += (double)ev[3] * (double)ev[3] + (double)ev[4] * (double)ev[4] + (double)ev[5] * (double)ev[5];
  }
  store_half_sum(acc, err + b);
}

// SE2 records: thx_se2_retract's arithmetic (step * delta in the run's dtype, exp and the product in fp64, csrc/pg3_generic.cuh);
// velocity records: x + step * delta, pad 0; masked problems copy the record
template <typename T>
__global__ void __launch_bounds__(256)
trajse2_retract_kernel(const T* __restrict__ x, const uint8_t* __restrict__ var_kind, const T* __restrict__ delta, int64_t ldd,
                       T step, const uint8_t* __restrict__ ignore, T* __restrict__ out, int V, int B, Eps2<double> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)V * B) return;
  const int k = (int)(gid / B), b = (int)(gid % B);
  const SE2<T> r = tse2_load(x, gid);
  if (ignore && ignore[b]) {
    tse2_store(out, gid, r.x, r.y, r.c, r.s);
    return;
  }
  const T* d = delta + (int64_t)b * ldd + 3 * k;
  const T d0 = d[0] * step, d1 = d[1] * step, d2 = d[2] * step;
  if (var_kind[k]) {
    tse2_store(out, gid, r.x + d0, r.y + d1, r.c + d2, (T)0);
    return;
  }
  const double xi[3] = {(double)d0, (double)d1, (double)d2};
  SE2<double> Ex, Y;
  se2_exp<double>(xi, eps, Ex, nullptr);
  se2_mul(SE2<double>{(double)r.x, (double)r.y, (double)r.c, (double)r.s}, Ex, Y);
  tse2_store(out, gid, (T)Y.x, (T)Y.y, (T)Y.c, (T)Y.s);
}

template <typename T>
inline Eps2<T> tse2_eps(const thx_se2_eps* e) {
  return Eps2<T>{(T)e->near_zero, (T)e->d_near_zero};
}

}  // namespace thx

using namespace thx;

extern "C" int thx_trajse2_eval(const thx_trajse2_term* terms, int32_t n_terms, const void* x, int32_t V, void* J, int64_t j_total,
                                void* e, int64_t lde, int32_t m, int32_t B, int dtype, const thx_se2_eps* eps, void* stream) {
  const char* who = "thx_trajse2_eval";
  unsigned blocks = 0;
  // (the state is read one 4-element record per load)
  if (int rc = family_check(who, !J || !e || !eps, terms, n_terms, x, 4, B, dtype, V < 1 ? ": V < 1" : nullptr)) return rc;
  if (int rc = family_check_eval(who, J, j_total < 3 ? ": j_total < 3" : nullptr, e, lde, m, n_terms, B, dtype, &blocks)) return rc;
  const dim3 grid(blocks), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(trajse2_eval_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, (const float*)x, V,
                                  (float*)J, j_total, (float*)e, lde, m, B, tse2_eps<float>(eps)),
               hipLaunchKernelGGL(trajse2_eval_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, (const double*)x,
                                  V, (double*)J, j_total, (double*)e, lde, m, B, tse2_eps<double>(eps)));
  return check_launch(who);
}

extern "C" int thx_trajse2_error(const thx_trajse2_term* terms, int32_t n_terms, const void* x, int32_t V, void* err, int32_t B,
                                 int dtype, const thx_se2_eps* eps, void* stream) {
  const char* who = "thx_trajse2_error";
  if (int rc = family_check(who, !err || !eps, terms, n_terms, x, 4, B, dtype, V < 1 ? ": V < 1" : nullptr)) return rc;
  if (reinterpret_cast<uintptr_t>(err) % (dtype == THX_F32 ? 4 : 8)) return fail(who, ": pointer not aligned");
  const dim3 grid((unsigned)B), block(kErrThreads);   // (B <= INT32_MAX: within the grid limit of the x dimension)
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(trajse2_error_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, (const float*)x,
                                  V, (float*)err, B, tse2_eps<float>(eps)),
               hipLaunchKernelGGL(trajse2_error_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms,
                                  (const double*)x, V, (double*)err, B, tse2_eps<double>(eps)));
  return check_launch(who);
}

extern "C" int thx_trajse2_retract(const void* x, const uint8_t* var_kind, const void* delta, int64_t ldd, double step,
                                   const uint8_t* ignore_mask, void* out, int32_t V, int32_t B, int dtype, const thx_se2_eps* eps,
                                   void* stream) {
  const char* who = "thx_trajse2_retract";
  if (!x || !var_kind || !delta || !out || !eps) return fail(who, ": null pointer");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (V < 1) return fail(who, ": V < 1");
  if (B < 1) return fail(who, ": empty batch");
  if (ldd < (int64_t)3 * V) return fail(who, ": ldd < 3 * V");
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  if (reinterpret_cast<uintptr_t>(x) % (4 * el) || reinterpret_cast<uintptr_t>(out) % (4 * el) || reinterpret_cast<uintptr_t>(delta) % el)
    return fail(who, ": pointer not aligned");
  const int64_t total = ((int64_t)V * B + 255) / 256;
  if (total > (int64_t)INT32_MAX) return fail(who, ": grid limit exceeded (V * B)");
  // the reference compares an fp32 angle with the fp32-rounded threshold (as thx_se2_retract)
  const Eps2<double> e2 = dtype == THX_F32 ? Eps2<double>{(double)(float)eps->near_zero, (double)(float)eps->d_near_zero}
                                           : Eps2<double>{eps->near_zero, eps->d_near_zero};
  const dim3 grid((unsigned)total), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(trajse2_retract_kernel<float>, grid, block, 0, as_stream(stream), (const float*)x, var_kind,
                                  (const float*)delta, ldd, (float)step, ignore_mask, (float*)out, V, B, e2),
               hipLaunchKernelGGL(trajse2_retract_kernel<double>, grid, block, 0, as_stream(stream), (const double*)x, var_kind,
                                  (const double*)delta, ldd, step, ignore_mask, (double*)out, V, B, e2));
  return check_launch(who);
}
