// Backward of pose graphs (SE3, SE2, SO3, SO2): three kernel templates over a group adapter G.
//
// BackwardMode.IMPLICIT (theseus/optimizer/nonlinear/nonlinear_least_squares.py:121-135, 265-292): the grad-enabled last step is
// X_new = X exp(delta),  delta = H^-1 g(theta)  with H detached (dense_linearization.py:61), theta = measurements / prior targets /
// cost weights.  Backward:
//   1. thx_*_retract_vjp : grad_delta = d/d delta < grad_X_new , X exp(step * delta) >          (retract_vjp_kernel)
//   2. thx_chol_solve    : w = H^-1 grad_delta with the cached factor (chol_kernels.hip)
//   3. thx_pg*_vjp       : grad_theta = d(w^T g)/d theta, per cost                               (pg_vjp_kernel)
// With q = w_j - Ad(D^-1) w_i (edges, D = v0^-1 v1; q = w_p for priors) the part of w^T g that belongs to one cost is
//   phi = - m(x, log_radius) sum_r s_r^2 (Jlog(E) q)_r log(E)_r ,   E = Z^-1 C   (Z = measurement, C = D | Z = target, C = var)
// RobustCostFunction (robust_cost_function.py:115-135) multiplies the cost's part by m = rho'(x) + 1e-20, x = sum_r (s_r log(E)_r)^2,
// which is NOT detached: d(m phi) = m d phi + phi (m_x dx + m_l d log_radius).
//
// BackwardMode.UNROLL / TRUNCATED: thx_pg*_unroll_vjp is the per-cost VJP of one differentiated iteration (unroll_se3.cuh states
// the maths; unroll_g3.cuh and vjp_so2.cuh are its 3-dof and 1-dof twins)                    (unroll_vjp_kernel)
//
// Every kernel: 64 lanes, grid (ceil(B / 64), costs | poses), one lane per (cost or pose, problem), batch index fastest across the
// wave; fp64 registers whatever the storage type; per-cost outputs, no atomics (the host sums the pose gradients of the unrolled
// backward in a fixed order: bit-reproducible).
//
// G provides:  DOF, REC (scalars per record), X (group element in fp64 registers), Eps (Taylor thresholds, rounded to the storage
//              type by eps()), HostEps (their C ABI struct; void: none), load, relative (C = Xi^-1 Xj and q), cost_vjp,
//              retract_vjp (hands each of the DOF values, before the common * step, to the kernel's store), unroll_vjp<EDGE>.
#include <type_traits>

#include "common.cuh"
#include "unroll_g3.cuh"
#include "unroll_se3.cuh"
#include "vjp_se3.cuh"
#include "vjp_so2.cuh"

namespace thx {

// the reference compares an fp32 angle with the fp32-rounded threshold
static inline Eps<double> lie_eps_rounded(const thx_lie_eps* e, int dtype) {
  return dtype == THX_F32 ? Eps<double>{(double)(float)e->near_zero, (double)(float)e->d_near_zero, (double)(float)e->near_pi}
                          : Eps<double>{e->near_zero, e->d_near_zero, e->near_pi};
}

// ---- SE3 ------------------------------------------------------------------------------------------------------------------------
// torchlie's SE3 backward semantics: Exp.backward (se3_impl.py:313-343, after Compose.backward :739-747)
//   grad_delta = Jexp(delta)^T [ Y_R^T G_t ; vee(Y_R^T G_R) ];
// d phi / d Z_k (12 raw entries) uses dual numbers through inverse / compose / the Jlog closed forms -- the derivative the
// reference's plain autograd takes -- while log(E)'s own derivative is torchlie's passthrough backward (se3_impl.py:487-493):
// d log = Jlog [E_R^T dE_t ; vee(E_R^T dE_R)/2]  (vjp_se3.cuh, unroll_se3.cuh).
struct VjpSE3 {
  static constexpr int DOF = 6, REC = 12;
  using X = SE3<double>;
  using Eps = thx::Eps<double>;
  using HostEps = thx_lie_eps;
  static Eps eps(const HostEps* e, int dtype) { return lie_eps_rounded(e, dtype); }

  template <typename T>
  static __device__ __forceinline__ void load(const T* __restrict__ p, X& x) {
    load_se3_any(p, x);
  }
  static __device__ __forceinline__ void relative(const X& Xi, const X& Xj, const double* wi, const double* wj, X& C, double* q) {
    X Xii, Di;
    se3_inv(Xi, Xii);
    se3_mul(Xii, Xj, C);
    se3_inv(C, Di);
    // q = w_j - Ad(D^-1) w_i,  Ad = [[R, hat(t) R],[0, R]]
    double Rl[3], Ra[3], tx[3];
    mat3_vec(Di.R, wi, Rl);
    mat3_vec(Di.R, wi + 3, Ra);
    cross3(Di.t, Ra, tx);  // hat(t) (R w_ang)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      q[k] = wj[k] - (Rl[k] + tx[k]);
      q[3 + k] = wj[3 + k] - Ra[k];
    }
  }
  static __device__ __forceinline__ void cost_vjp(const X& Z, const X& C, const double* q, const double* s, const Eps& eps, int loss,
                                                  double lr, double* gZ, double* gs, double* glr) {
    thx::cost_vjp(Z, C, q, s, eps, loss, lr, gZ, gs, glr);
  }
  template <typename Store>
  static __device__ __forceinline__ void retract_vjp(const X& Xv, const X& G, const double* xi, const Eps& eps, Store out) {
    X Ex, Y;
    ExpCoef<double> c;
    double Ct, J[36];
    se3_exp(xi, eps, Ex, c, Ct);
    se3_jexp(xi, Ex, c, Ct, J);
    se3_mul(Xv, Ex, Y);
    double M[9], u[6];
    mat3_tmul(Y.R, G.R, M);
    mat3_tvec(Y.R, G.t, u);
    u[3] = M[7] - M[5];
    u[4] = M[2] - M[6];
    u[5] = M[3] - M[1];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) acc += J[6 * k + i] * u[k];
      out(i, acc);
    }
  }
  template <bool EDGE>
  static __device__ __forceinline__ void unroll_vjp(const X& Xi, const X& Xj, const X& Z, const double* s, const double* wi,
                                                    const double* wj, const double* di, const double* dj, const Eps& eps,
                                                    double lam, int loss, double lr, double* g, double* gs, double* glr) {
    if (EDGE) unroll_edge_vjp(Xi, Xj, Z, s, wi, wj, di, dj, eps, g, g + REC, g + 2 * REC, gs, lam, loss, lr, glr);
    else unroll_prior_vjp(Xj, Z, s, wj, dj, eps, g + REC, g + 2 * REC, gs, lam, loss, lr, glr);
  }
};

// ---- SE2 ------------------------------------------------------------------------------------------------------------------------
// theseus/geometry/se2.py has no custom backward anywhere (plain autograd through the closed forms, atan2 included), so every
// derivative is the dual part of the SAME templated arithmetic (lie_se2.cuh on Dual<double>, Taylor branches included).

// per row r: phi_r = - s_r^2 (Jlog q)_r xi_r (phi_plain = sum_r phi_r) and x_r = (s_r xi_r)^2 for E = Z^-1 C, on any scalar type
template <typename S>
__device__ __forceinline__ void cost_phi2(const SE2<S>& Z, const SE2<S>& C, const double* q, const double* s, const Eps2<S>& eps,
                                          S* phi_r, S* x_r, S* a_out, S* xi_out) {
  SE2<S> Zi, E;
  se2_inv(Z, Zi);
  se2_mul(Zi, C, E);
  S xi[3], J[9];
  se2_log_jlog(E, eps, xi, J, true);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const S a = J[3 * r] * S(q[0]) + J[3 * r + 1] * S(q[1]) + J[3 * r + 2] * S(q[2]);
    phi_r[r] = S(0.0) - S(s[r] * s[r]) * a * xi[r];
    x_r[r] = S(s[r] * s[r]) * xi[r] * xi[r];
    if (a_out) { a_out[r] = a; xi_out[r] = xi[r]; }
  }
}

__device__ __forceinline__ void cost_vjp2(const SE2<double>& Z, const SE2<double>& C, const double* q, const double* s,
                                          const Eps2<double>& eps, int loss, double log_radius, double* gZ, double* gs,
                                          double* glr) {
  double phi_r[3], x_r[3], Phi[3], a[3], xi[3];
  cost_phi2<double>(Z, C, q, s, eps, phi_r, x_r, a, xi);
  RobustTerms<3> rt;   // robust.cuh
  rt.eval(loss, x_r, log_radius);
  rt.group(phi_r, Phi);
  double gl = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    gl += phi_r[r] * rt.m_l[r];
    gs[r] = rt.m[r] * (-2.0 * s[r] * a[r] * xi[r]) + Phi[r] * rt.m_x[r] * (2.0 * s[r] * xi[r] * xi[r]);
  }
  *glr = gl;
  const Eps2<D2> epsd{D2(eps.nz), D2(eps.dnz)};
  const SE2<D2> Cd{D2(C.x), D2(C.y), D2(C.c), D2(C.s)};
  for (int k = 0; k < 4; ++k) {  // one dual evaluation per raw entry [x, y, cos, sin] of Z
    const SE2<D2> Zd{D2(Z.x, k == 0 ? 1.0 : 0.0), D2(Z.y, k == 1 ? 1.0 : 0.0), D2(Z.c, k == 2 ? 1.0 : 0.0),
                     D2(Z.s, k == 3 ? 1.0 : 0.0)};
    D2 phid[3], xd[3];
    cost_phi2<D2>(Zd, Cd, q, s, epsd, phid, xd, nullptr, nullptr);
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) g += rt.m[r] * phid[r].d + Phi[r] * rt.m_x[r] * xd[r].d;
    gZ[k] = g;
  }
}

struct VjpSE2 {
  static constexpr int DOF = 3, REC = 4;
  using X = SE2<double>;
  using Eps = Eps2<double>;
  using HostEps = thx_se2_eps;
  static Eps eps(const HostEps* e, int dtype) {
    return dtype == THX_F32 ? Eps{(double)(float)e->near_zero, (double)(float)e->d_near_zero} : Eps{e->near_zero, e->d_near_zero};
  }

  template <typename T>
  static __device__ __forceinline__ void load(const T* __restrict__ p, X& x) {
    x = X{(double)p[0], (double)p[1], (double)p[2], (double)p[3]};
  }
  static __device__ __forceinline__ void relative(const X& Xi, const X& Xj, const double* wi, const double* wj, X& C, double* q) {
    X Xii, Di;
    se2_inv(Xi, Xii);
    se2_mul(Xii, Xj, C);
    se2_inv(C, Di);
    double Ad[9];
    se2_adjoint(Di, Ad);
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = wj[r] - (Ad[3 * r] * wi[0] + Ad[3 * r + 1] * wi[1] + Ad[3 * r + 2] * wi[2]);
  }
  static __device__ __forceinline__ void cost_vjp(const X& Z, const X& C, const double* q, const double* s, const Eps& eps, int loss,
                                                  double lr, double* gZ, double* gs, double* glr) {
    cost_vjp2(Z, C, q, s, eps, loss, lr, gZ, gs, glr);
  }
  // grad_delta_k = < grad_X_new , d/d delta_k [ X exp(step * delta) ] >
  template <typename Store>
  static __device__ __forceinline__ void retract_vjp(const X& Xv, const X& G, const double* xi, const Eps& eps, Store out) {
    const Eps2<D2> epsd{D2(eps.nz), D2(eps.dnz)};
    const SE2<D2> Xd{D2(Xv.x), D2(Xv.y), D2(Xv.c), D2(Xv.s)};
    for (int k = 0; k < 3; ++k) {
      const D2 xid[3] = {D2(xi[0], k == 0 ? 1.0 : 0.0), D2(xi[1], k == 1 ? 1.0 : 0.0), D2(xi[2], k == 2 ? 1.0 : 0.0)};
      SE2<D2> Ex, Y;
      se2_exp<D2>(xid, epsd, Ex, nullptr);
      se2_mul(Xd, Ex, Y);
      out(k, G.x * Y.x.d + G.y * Y.y.d + G.c * Y.c.d + G.s * Y.s.d);
    }
  }
  template <bool EDGE>
  static __device__ __forceinline__ void unroll_vjp(const X& Xi, const X& Xj, const X& Z, const double* s, const double* wi,
                                                    const double* wj, const double* di, const double* dj, const Eps& eps,
                                                    double lam, int loss, double lr, double* g, double* gs, double* glr) {
    const double ri[4] = {Xi.x, Xi.y, Xi.c, Xi.s}, rj[4] = {Xj.x, Xj.y, Xj.c, Xj.s}, rz[4] = {Z.x, Z.y, Z.c, Z.s};
    unroll3_vjp<UG_SE2, EDGE>(ri, rj, rz, s, wi, wj, di, dj, eps, lam, loss, lr, g, gs, glr);
  }
};

// ---- SO3 ------------------------------------------------------------------------------------------------------------------------
// torchlie's SO3 backward semantics (torchlie/torchlie/functional/so3_impl.py): Exp.backward (:336-353) grad_w = Jexp^T vee2(R^T G);
// Log's passthrough backward (:489-496) d log = Jlog vee2(E^T dE) / 2 -- the tangent projection, not the derivative of the closed
// form; Inverse / Compose (:576-577, :702-707) are the plain matrix derivatives; the Jlog closed forms are differentiated by plain
// autograd (dual numbers through so3_log_jlog, Taylor branches included).  vee2(M) = (M21 - M12, M02 - M20, M10 - M01).

// gradient of phi w.r.t. the 9 raw entries of Z (row major), the 3 weights and log_radius
__device__ __forceinline__ void cost_vjp_so3(const double* Z, const double* C, const double* q, const double* s,
                                             const Eps<double>& eps, int loss, double log_radius, double* gZ, double* gs,
                                             double* glr) {
  double E[9], xi[3], J[9], a[3];
  mat3_tmul(Z, C, E);
  so3_log_jlog<double>(E, eps, xi, J, true);
  mat3_vec(J, q, a);
  double phi_r[3], x_r[3], Phi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    phi_r[r] = -s[r] * s[r] * a[r] * xi[r];
    x_r[r] = (s[r] * xi[r]) * (s[r] * xi[r]);
  }
  RobustTerms<3> rt;   // robust.cuh
  rt.eval(loss, x_r, log_radius);
  rt.group(phi_r, Phi);
  double gl = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    gl += phi_r[r] * rt.m_l[r];
    gs[r] = rt.m[r] * (-2.0 * s[r] * a[r] * xi[r]) + Phi[r] * rt.m_x[r] * (2.0 * s[r] * xi[r] * xi[r]);
  }
  *glr = gl;
  const Eps<D2> epsd{D2(eps.nz), D2(eps.dnz), D2(eps.npi)};
  D2 Cd[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Cd[i] = D2(C[i]);
  for (int k = 0; k < 9; ++k) {  // run-time loop: one dual evaluation per raw entry of Z
    D2 Zd[9], Ed[9], xid[3], Jd[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Zd[i] = D2(Z[i], i == k ? 1.0 : 0.0);
    mat3_tmul(Zd, Cd, Ed);
    so3_log_jlog<D2>(Ed, epsd, xid, Jd, true);
    // torchlie's log backward: d xi = Jlog vee2(E^T dE) / 2
    double dE[9], M[9], u[3], dxi[3], da[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) dE[i] = Ed[i].d;
    mat3_tmul(E, dE, M);
    u[0] = 0.5 * (M[7] - M[5]);
    u[1] = 0.5 * (M[2] - M[6]);
    u[2] = 0.5 * (M[3] - M[1]);
    mat3_vec(J, u, dxi);
#pragma unroll
    for (int i = 0; i < 3; ++i) da[i] = Jd[3 * i].d * q[0] + Jd[3 * i + 1].d * q[1] + Jd[3 * i + 2].d * q[2];
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      g += rt.m[r] * (-s[r] * s[r] * (da[r] * xi[r] + a[r] * dxi[r])) + Phi[r] * rt.m_x[r] * (2.0 * s[r] * s[r] * xi[r] * dxi[r]);
    gZ[k] = g;
  }
}

struct VjpSO3 {
  static constexpr int DOF = 3, REC = 9;
  using X = SO3m<double>;
  using Eps = thx::Eps<double>;
  using HostEps = thx_lie_eps;
  static Eps eps(const HostEps* e, int dtype) { return lie_eps_rounded(e, dtype); }

  template <typename T>
  static __device__ __forceinline__ void load(const T* __restrict__ p, X& x) {
#pragma unroll
    for (int k = 0; k < 9; ++k) x.R[k] = (double)p[k];
  }
  static __device__ __forceinline__ void relative(const X& Xi, const X& Xj, const double* wi, const double* wj, X& C, double* q) {
    mat3_tmul(Xi.R, Xj.R, C.R);
    double Dtw[3];
    mat3_tvec(C.R, wi, Dtw);  // Ad(D^-1) w_i = D^T w_i
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = wj[r] - Dtw[r];
  }
  static __device__ __forceinline__ void cost_vjp(const X& Z, const X& C, const double* q, const double* s, const Eps& eps, int loss,
                                                  double lr, double* gZ, double* gs, double* glr) {
    cost_vjp_so3(Z.R, C.R, q, s, eps, loss, lr, gZ, gs, glr);
  }
  // grad_delta = Jexp(step delta)^T vee2(Y^T G),  Y = X exp(step delta)
  template <typename Store>
  static __device__ __forceinline__ void retract_vjp(const X& Xv, const X& G, const double* xi, const Eps& eps, Store out) {
    double J[9], Y[9], M[9], u[3];
    GroupSO3::X Ex;
    GroupSO3::exp(xi, eps, Ex, J);
    mat3_mul(Xv.R, Ex.R, Y);
    mat3_tmul(Y, G.R, M);
    u[0] = M[7] - M[5];
    u[1] = M[2] - M[6];
    u[2] = M[3] - M[1];
#pragma unroll
    for (int i = 0; i < 3; ++i) out(i, J[i] * u[0] + J[3 + i] * u[1] + J[6 + i] * u[2]);
  }
  template <bool EDGE>
  static __device__ __forceinline__ void unroll_vjp(const X& Xi, const X& Xj, const X& Z, const double* s, const double* wi,
                                                    const double* wj, const double* di, const double* dj, const Eps& eps,
                                                    double lam, int loss, double lr, double* g, double* gs, double* glr) {
    unroll3_vjp<UG_SO3, EDGE>(Xi.R, Xj.R, Z.R, s, wi, wj, di, dj, eps, lam, loss, lr, g, gs, glr);
  }
};

// ---- SO2 ------------------------------------------------------------------------------------------------------------------------
// theseus/geometry/so2.py has no custom backward: plain autograd through its closed forms, on dual numbers (vjp_so2.cuh states the
// maths).  No Taylor thresholds.
struct VjpSO2 {
  static constexpr int DOF = 1, REC = 2;
  using X = SO2r<double>;
  struct Eps {};
  using HostEps = void;
  static Eps eps(const HostEps*, int) { return Eps{}; }

  template <typename T>
  static __device__ __forceinline__ void load(const T* __restrict__ p, X& x) {
    x = X{(double)p[0], (double)p[1]};
  }
  static __device__ __forceinline__ void relative(const X& Xi, const X& Xj, const double* wi, const double* wj, X& C, double* q) {
    C = so2r_mul(so2r_inv(Xi), Xj);
    q[0] = wj[0] - wi[0];   // Ad = 1
  }
  static __device__ __forceinline__ void cost_vjp(const X& Z, const X& C, const double* q, const double* s, const Eps&, int loss,
                                                  double lr, double* gZ, double* gs, double* glr) {
    const double z[2] = {Z.c, Z.s}, c[2] = {C.c, C.s};
    so2_cost_vjp(z, c, q[0], s[0], loss, lr, gZ, gs, glr);
  }
  template <typename Store>
  static __device__ __forceinline__ void retract_vjp(const X& Xv, const X& G, const double* xi, const Eps&, Store out) {
    const double x[2] = {Xv.c, Xv.s}, g[2] = {G.c, G.s};
    out(0, so2_retract_vjp(x, g, xi[0]));
  }
  template <bool EDGE>
  static __device__ __forceinline__ void unroll_vjp(const X& Xi, const X& Xj, const X& Z, const double* s, const double* wi,
                                                    const double* wj, const double* di, const double* dj, const Eps&, double lam,
                                                    int loss, double lr, double* g, double* gs, double* glr) {
    const double ri[2] = {Xi.c, Xi.s}, rj[2] = {Xj.c, Xj.s}, rz[2] = {Z.c, Z.s};
    so2_unroll_vjp<EDGE>(ri, rj, rz, s[0], wi[0], wj[0], di[0], dj[0], lam, loss, lr, g, gs, glr);
  }
};

// ---- kernels --------------------------------------------------------------------------------------------------------------------

template <typename G, typename T>
__global__ void __launch_bounds__(64)
pg_vjp_kernel(thx_pg_structure s, thx_pg_data d, const T* __restrict__ wvec, int64_t ldw, T* __restrict__ g_meas,
              T* __restrict__ g_wb, T* __restrict__ g_tgt, T* __restrict__ g_wp, T* __restrict__ g_lrb, T* __restrict__ g_lrp,
              typename G::Eps eps) {
  constexpr int N = G::DOF, R = G::REC;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y;
  const int B = d.batch;
  if (b >= B) return;
  const T* poses = static_cast<const T*>(d.poses);
  const T* wv = wvec + (int64_t)b * ldw;
  double q[N], sw[N], gZ[R], gs[N], glr = 0.0, lr = 0.0;
  int loss = THX_LOSS_NONE;
  typename G::X Z, C;
  T *outZ, *outS, *outL = nullptr;
  if (c < s.num_edges) {
    const int e = c, i = s.edge_i[e], j = s.edge_j[e];
    const int64_t mB = d.meas_bstride ? B : 1, wB = d.w_between_bstride ? B : 1;
    typename G::X Xi, Xj;
    G::load(poses + ((int64_t)i * B + b) * R, Xi);
    G::load(poses + ((int64_t)j * B + b) * R, Xj);
    G::load(static_cast<const T*>(d.meas) + ((int64_t)e * mB) * R + (int64_t)b * d.meas_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_between) + ((int64_t)e * wB) * N + (int64_t)b * d.w_between_bstride;
    double wi[N], wj[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      wi[k] = (double)wv[N * i + k];
      wj[k] = (double)wv[N * j + k];
      sw[k] = (double)wp[k];
    }
    G::relative(Xi, Xj, wi, wj, C, q);  // C = D = v0^-1 v1
    outZ = g_meas + ((int64_t)e * B + b) * R;
    outS = g_wb + ((int64_t)e * B + b) * N;
    loss = loss_code(d.robust_between, d.loss_between, e);
    if (loss) lr = load_log_radius<T>(d.log_radius_between, e, b, B, d.log_radius_between_bstride);
    if (d.robust_between) outL = g_lrb ? g_lrb + (int64_t)e * B + b : nullptr;   // (a plain cost of a mixed role: 0)
  } else {
    const int k = c - s.num_edges, p = s.prior_pose[k];
    const int64_t tB = d.prior_target_bstride ? B : 1, wB = d.w_prior_bstride ? B : 1;
    G::load(poses + ((int64_t)p * B + b) * R, C);
    G::load(static_cast<const T*>(d.prior_target) + ((int64_t)k * tB) * R + (int64_t)b * d.prior_target_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_prior) + ((int64_t)k * wB) * N + (int64_t)b * d.w_prior_bstride;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      q[r] = (double)wv[N * p + r];
      sw[r] = (double)wp[r];
    }
    outZ = g_tgt + ((int64_t)k * B + b) * R;
    outS = g_wp + ((int64_t)k * B + b) * N;
    loss = loss_code(d.robust_prior, d.loss_prior, k);
    if (loss) lr = load_log_radius<T>(d.log_radius_prior, k, b, B, d.log_radius_prior_bstride);
    if (d.robust_prior) outL = g_lrp ? g_lrp + (int64_t)k * B + b : nullptr;
  }
  G::cost_vjp(Z, C, q, sw, eps, loss, lr, gZ, gs, &glr);
  if (outL) *outL = (T)glr;
#pragma unroll
  for (int k = 0; k < R; ++k) outZ[k] = (T)gZ[k];
#pragma unroll
  for (int k = 0; k < N; ++k) outS[k] = (T)gs[k];
}

template <typename G, typename T>
__global__ void __launch_bounds__(64)
retract_vjp_kernel(const T* __restrict__ poses, const T* __restrict__ delta, int64_t ldd, T step, const T* __restrict__ gout,
                   T* __restrict__ gdelta, int64_t ldg, int P, int B, typename G::Eps eps) {
  constexpr int N = G::DOF, R = G::REC;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B) return;
  typename G::X X, Gx;   // Gx: the raw gradient of X_new, read as a record
  G::load(poses + ((int64_t)p * B + b) * R, X);
  G::load(gout + ((int64_t)p * B + b) * R, Gx);
  double xi[N];
#pragma unroll
  for (int i = 0; i < N; ++i) xi[i] = (double)(delta[(int64_t)b * ldd + N * p + i] * step);
  G::retract_vjp(X, Gx, xi, eps, [&](int i, double v) { gdelta[(int64_t)b * ldg + N * p + i] = (T)(v * (double)step); });
}

template <typename G, typename T>
__global__ void __launch_bounds__(64)
unroll_vjp_kernel(thx_pg_structure s, thx_pg_data d, const T* __restrict__ wvec, int64_t ldw, const T* __restrict__ dvec,
                  int64_t ldd, const T* __restrict__ ell_damping, T* __restrict__ g_pose_i, T* __restrict__ g_pose_j,
                  T* __restrict__ g_meas, T* __restrict__ g_wb, T* __restrict__ g_pose_p, T* __restrict__ g_tgt,
                  T* __restrict__ g_wp, T* __restrict__ g_lrb, T* __restrict__ g_lrp, typename G::Eps eps) {
  constexpr int N = G::DOF, R = G::REC;
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y;
  const int B = d.batch;
  if (b >= B) return;
  const T* poses = static_cast<const T*>(d.poses);
  const T* wv = wvec + (int64_t)b * ldw;
  const T* dv = dvec + (int64_t)b * ldd;
  const double lam = ell_damping ? (double)ell_damping[b] : 0.0;   // ellipsoidal damping: lambda_b (null: spherical / none)
  // g: [0, R) w.r.t. Xi, [R, 2R) Xj (the prior's variable), [2R, 3R) Z (the prior's target)
  double sw[N], wi[N] = {}, wj[N], di[N] = {}, dj[N], g[3 * R], gs[N], glr = 0.0;
  typename G::X Xi, Xj, Z;
  if (c < s.num_edges) {
    const int e = c, i = s.edge_i[e], j = s.edge_j[e];
    const int64_t mB = d.meas_bstride ? B : 1, wB = d.w_between_bstride ? B : 1;
    G::load(poses + ((int64_t)i * B + b) * R, Xi);
    G::load(poses + ((int64_t)j * B + b) * R, Xj);
    G::load(static_cast<const T*>(d.meas) + ((int64_t)e * mB) * R + (int64_t)b * d.meas_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_between) + ((int64_t)e * wB) * N + (int64_t)b * d.w_between_bstride;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      wi[k] = (double)wv[N * i + k];
      wj[k] = (double)wv[N * j + k];
      di[k] = (double)dv[N * i + k];
      dj[k] = (double)dv[N * j + k];
      sw[k] = (double)wp[k];
    }
    const int loss = loss_code(d.robust_between, d.loss_between, e);
    const double lr = loss ? load_log_radius<T>(d.log_radius_between, e, b, B, d.log_radius_between_bstride) : 0.0;
    G::template unroll_vjp<true>(Xi, Xj, Z, sw, wi, wj, di, dj, eps, lam, loss, lr, g, gs, &glr);
    T* oi = g_pose_i + ((int64_t)e * B + b) * R;
    T* oj = g_pose_j + ((int64_t)e * B + b) * R;
    T* oz = g_meas + ((int64_t)e * B + b) * R;
    T* os = g_wb + ((int64_t)e * B + b) * N;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      oi[k] = (T)g[k];
      oj[k] = (T)g[R + k];
      oz[k] = (T)g[2 * R + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) os[k] = (T)gs[k];
    if (d.robust_between && g_lrb) g_lrb[(int64_t)e * B + b] = (T)glr;   // (a plain cost of a mixed role: 0)
  } else {
    const int k0 = c - s.num_edges, p = s.prior_pose[k0];
    const int64_t tB = d.prior_target_bstride ? B : 1, wB = d.w_prior_bstride ? B : 1;
    G::load(poses + ((int64_t)p * B + b) * R, Xj);
    G::load(static_cast<const T*>(d.prior_target) + ((int64_t)k0 * tB) * R + (int64_t)b * d.prior_target_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_prior) + ((int64_t)k0 * wB) * N + (int64_t)b * d.w_prior_bstride;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      wj[r] = (double)wv[N * p + r];
      dj[r] = (double)dv[N * p + r];
      sw[r] = (double)wp[r];
    }
    const int loss = loss_code(d.robust_prior, d.loss_prior, k0);
    const double lr = loss ? load_log_radius<T>(d.log_radius_prior, k0, b, B, d.log_radius_prior_bstride) : 0.0;
    G::template unroll_vjp<false>(Xj, Xj, Z, sw, wi, wj, di, dj, eps, lam, loss, lr, g, gs, &glr);
    T* ox = g_pose_p + ((int64_t)k0 * B + b) * R;
    T* ot = g_tgt + ((int64_t)k0 * B + b) * R;
    T* os = g_wp + ((int64_t)k0 * B + b) * N;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      ox[k] = (T)g[R + k];
      ot[k] = (T)g[2 * R + k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) os[k] = (T)gs[k];
    if (d.robust_prior && g_lrp) g_lrp[(int64_t)k0 * B + b] = (T)glr;
  }
}

// ---- launchers: the argument checks once, then the float or double instantiation ------------------------------------------------

template <typename G>
static bool eps_missing(const typename G::HostEps* eps) {
  return !std::is_void<typename G::HostEps>::value && !eps;
}

template <typename G>
static int launch_pg_vjp(const char* name, const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* gm,
                         void* gwb, void* gt, void* gwp, void* glb, void* glp, int dtype, const typename G::HostEps* eps,
                         void* stream) {
  if (!s || !d || !w || eps_missing<G>(eps)) return fail(name, ": null argument");
  if (s->num_edges > 0 && (!gm || !gwb)) return fail(name, ": null edge gradient buffer");
  if (s->num_priors > 0 && (!gt || !gwp)) return fail(name, ": null prior gradient buffer");
  if (ldw < G::DOF * (int64_t)s->num_poses) return fail(name, ": ldw < n");
  if (const char* why = check_robust(d)) return fail(why);
  dim3 grid((d->batch + 63) / 64, s->num_edges + s->num_priors), block(64);
  if (grid.y == 0) return 0;
  const typename G::Eps e = G::eps(eps, dtype);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((pg_vjp_kernel<G, T>), grid, block, 0, as_stream(stream), *s, *d, (const T*)w, ldw, (T*)gm, (T*)gwb, (T*)gt,
                       (T*)gwp, (T*)glb, (T*)glp, e);
  };
  THX_DISPATCH(dtype, go(0.0f), go(0.0));
  return check_launch(name);
}

template <typename G>
static int launch_retract_vjp(const char* name, const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out,
                              void* grad_delta, int64_t ldg, int32_t P, int32_t B, int dtype, const typename G::HostEps* eps,
                              void* stream) {
  if (!poses || !delta || !grad_out || !grad_delta || eps_missing<G>(eps) || P <= 0 || B <= 0) return fail(name, ": bad arguments");
  dim3 grid((B + 63) / 64, P), block(64);
  const typename G::Eps e = G::eps(eps, dtype);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((retract_vjp_kernel<G, T>), grid, block, 0, as_stream(stream), (const T*)poses, (const T*)delta, ldd, (T)step,
                       (const T*)grad_out, (T*)grad_delta, ldg, P, B, e);
  };
  THX_DISPATCH(dtype, go(0.0f), go(0.0));
  return check_launch(name);
}

template <typename G>
static int launch_unroll_vjp(const char* name, const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw,
                             const void* delta, int64_t ldd, const void* ell, void* gpi, void* gpj, void* gm, void* gwb, void* gpp,
                             void* gt, void* gwp, void* glb, void* glp, int dtype, const typename G::HostEps* eps, void* stream) {
  if (!s || !d || !w || !delta || eps_missing<G>(eps)) return fail(name, ": null argument");
  if (s->num_edges > 0 && (!gpi || !gpj || !gm || !gwb)) return fail(name, ": null edge gradient buffer");
  if (s->num_priors > 0 && (!gpp || !gt || !gwp)) return fail(name, ": null prior gradient buffer");
  if (ldw < G::DOF * (int64_t)s->num_poses || ldd < G::DOF * (int64_t)s->num_poses) return fail(name, ": ldw / ldd < n");
  if (const char* why = check_robust(d)) return fail(why);
  dim3 grid((d->batch + 63) / 64, s->num_edges + s->num_priors), block(64);
  if (grid.y == 0) return 0;
  const typename G::Eps e = G::eps(eps, dtype);
  auto go = [&](auto zero) {
    using T = decltype(zero);
    hipLaunchKernelGGL((unroll_vjp_kernel<G, T>), grid, block, 0, as_stream(stream), *s, *d, (const T*)w, ldw, (const T*)delta, ldd,
                       (const T*)ell, (T*)gpi, (T*)gpj, (T*)gm, (T*)gwb, (T*)gpp, (T*)gt, (T*)gwp, (T*)glb, (T*)glp, e);
  };
  THX_DISPATCH(dtype, go(0.0f), go(0.0));
  return check_launch(name);
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_pg_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* grad_meas, void* grad_w_between,
               void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between, void* grad_log_radius_prior, int dtype,
               const thx_lie_eps* eps, void* stream) {
  return launch_pg_vjp<VjpSE3>("thx_pg_vjp", s, d, w, ldw, grad_meas, grad_w_between, grad_prior_target, grad_w_prior,
                               grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pg2_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* grad_meas, void* grad_w_between,
                void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between, void* grad_log_radius_prior, int dtype,
                const thx_se2_eps* eps, void* stream) {
  return launch_pg_vjp<VjpSE2>("thx_pg2_vjp", s, d, w, ldw, grad_meas, grad_w_between, grad_prior_target, grad_w_prior,
                               grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pgso3_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* grad_meas,
                  void* grad_w_between, void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between,
                  void* grad_log_radius_prior, int dtype, const thx_lie_eps* eps, void* stream) {
  return launch_pg_vjp<VjpSO3>("thx_pgso3_vjp", s, d, w, ldw, grad_meas, grad_w_between, grad_prior_target, grad_w_prior,
                               grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pgso2_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* grad_meas,
                  void* grad_w_between, void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between,
                  void* grad_log_radius_prior, int dtype, void* stream) {
  return launch_pg_vjp<VjpSO2>("thx_pgso2_vjp", s, d, w, ldw, grad_meas, grad_w_between, grad_prior_target, grad_w_prior,
                               grad_log_radius_between, grad_log_radius_prior, dtype, nullptr, stream);
}

int thx_se3_retract_vjp(const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out, void* grad_delta,
                        int64_t ldg, int32_t P, int32_t B, int dtype, const thx_lie_eps* eps, void* stream) {
  return launch_retract_vjp<VjpSE3>("thx_se3_retract_vjp", poses, delta, ldd, step, grad_out, grad_delta, ldg, P, B, dtype, eps,
                                    stream);
}

int thx_se2_retract_vjp(const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out, void* grad_delta,
                        int64_t ldg, int32_t P, int32_t B, int dtype, const thx_se2_eps* eps, void* stream) {
  return launch_retract_vjp<VjpSE2>("thx_se2_retract_vjp", poses, delta, ldd, step, grad_out, grad_delta, ldg, P, B, dtype, eps,
                                    stream);
}

int thx_so3_retract_vjp(const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out, void* grad_delta,
                        int64_t ldg, int32_t P, int32_t B, int dtype, const thx_lie_eps* eps, void* stream) {
  return launch_retract_vjp<VjpSO3>("thx_so3_retract_vjp", poses, delta, ldd, step, grad_out, grad_delta, ldg, P, B, dtype, eps,
                                    stream);
}

int thx_so2_retract_vjp(const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out, void* grad_delta,
                        int64_t ldg, int32_t P, int32_t B, int dtype, void* stream) {
  return launch_retract_vjp<VjpSO2>("thx_so2_retract_vjp", poses, delta, ldd, step, grad_out, grad_delta, ldg, P, B, dtype, nullptr,
                                    stream);
}

int thx_pg_unroll_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, const void* delta, int64_t ldd,
                      const void* ellipsoidal_damping, void* grad_pose_i, void* grad_pose_j, void* grad_meas, void* grad_w_between,
                      void* grad_pose_prior, void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between,
                      void* grad_log_radius_prior, int dtype, const thx_lie_eps* eps, void* stream) {
  return launch_unroll_vjp<VjpSE3>("thx_pg_unroll_vjp", s, d, w, ldw, delta, ldd, ellipsoidal_damping, grad_pose_i, grad_pose_j,
                                   grad_meas, grad_w_between, grad_pose_prior, grad_prior_target, grad_w_prior,
                                   grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pg2_unroll_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, const void* delta, int64_t ldd,
                       const void* ellipsoidal_damping, void* grad_pose_i, void* grad_pose_j, void* grad_meas, void* grad_w_between,
                       void* grad_pose_prior, void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between,
                       void* grad_log_radius_prior, int dtype, const thx_se2_eps* eps, void* stream) {
  return launch_unroll_vjp<VjpSE2>("thx_pg2_unroll_vjp", s, d, w, ldw, delta, ldd, ellipsoidal_damping, grad_pose_i, grad_pose_j,
                                   grad_meas, grad_w_between, grad_pose_prior, grad_prior_target, grad_w_prior,
                                   grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pgso3_unroll_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, const void* delta, int64_t ldd,
                         const void* ellipsoidal_damping, void* grad_pose_i, void* grad_pose_j, void* grad_meas,
                         void* grad_w_between, void* grad_pose_prior, void* grad_prior_target, void* grad_w_prior,
                         void* grad_log_radius_between, void* grad_log_radius_prior, int dtype, const thx_lie_eps* eps, void* stream) {
  return launch_unroll_vjp<VjpSO3>("thx_pgso3_unroll_vjp", s, d, w, ldw, delta, ldd, ellipsoidal_damping, grad_pose_i, grad_pose_j,
                                   grad_meas, grad_w_between, grad_pose_prior, grad_prior_target, grad_w_prior,
                                   grad_log_radius_between, grad_log_radius_prior, dtype, eps, stream);
}

int thx_pgso2_unroll_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, const void* delta, int64_t ldd,
                         const void* ellipsoidal_damping, void* grad_pose_i, void* grad_pose_j, void* grad_meas,
                         void* grad_w_between, void* grad_pose_prior, void* grad_prior_target, void* grad_w_prior,
                         void* grad_log_radius_between, void* grad_log_radius_prior, int dtype, void* stream) {
  return launch_unroll_vjp<VjpSO2>("thx_pgso2_unroll_vjp", s, d, w, ldw, delta, ldd, ellipsoidal_damping, grad_pose_i, grad_pose_j,
                                   grad_meas, grad_w_between, grad_pose_prior, grad_prior_target, grad_w_prior,
                                   grad_log_radius_between, grad_log_radius_prior, dtype, nullptr, stream);
}

}  // extern "C"
