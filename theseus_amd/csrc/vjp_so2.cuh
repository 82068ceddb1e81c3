// Backward maths of SO2 pose graphs (planar rotation-only graphs, theseus/geometry/so2.py): the 1-dof twins of pg_vjp_kernels.hip's
// cost_vjp2 (BackwardMode.IMPLICIT) and unroll_g3.cuh's unroll3_vjp (UNROLL / TRUNCATED).  so2.py has no custom backward: every
// derivative is plain autograd through its closed forms -- compose by the angle-addition formulas (:225-231), inverse (cos, -sin)
// (:233-235), log = atan2(sin, cos) (:206-223), exp = (cos theta, sin theta) (:167-186) -- so every derivative here is the dual part
// of that SAME arithmetic on Dual<double> (dual.cuh: t_atan2 carries (x dy - y dx) / (x^2 + y^2)).  Records are never
// re-normalised, so the off-manifold factor x^2 + y^2 stays in every pose / measurement gradient.  Jlog, Jexp and the adjoint are
// the constant 1 (so2.py:116-117, :180-185, :210-219: torch.ones, no graph), which is why they appear below as plain numbers.
// Plain C++ templates: also compiled for the host by tests/hostmath.
#pragma once
#include "dual.cuh"
#include "robust.cuh"

namespace thx {

using SD = Dual<double>;

template <typename S>
struct SO2r {
  S c, s;   // raw record [cos, sin]
};

template <typename S>
__device__ __forceinline__ SO2r<S> so2r_inv(const SO2r<S>& a) {
  return SO2r<S>{a.c, -a.s};
}
template <typename S>
__device__ __forceinline__ SO2r<S> so2r_mul(const SO2r<S>& a, const SO2r<S>& b) {
  return SO2r<S>{a.c * b.c - a.s * b.s, a.s * b.c + a.c * b.s};
}
template <typename S>
__device__ __forceinline__ S so2r_log(const SO2r<S>& x) {
  return t_atan2(x.s, x.c);
}
// raw entries as duals, the k-th one seeded (k < 0: none)
__device__ __forceinline__ SO2r<SD> so2r_seed(const double* raw, int k) {
  return SO2r<SD>{SD(raw[0], k == 0 ? 1.0 : 0.0), SD(raw[1], k == 1 ? 1.0 : 0.0)};
}

// ---- the retraction X exp(theta) (lie_group.py:197-198): d/dtheta < G , X exp(theta) > for the raw gradient G of the result ----
__device__ __forceinline__ double so2_retract_vjp(const double* X, const double* G, double theta) {
  const SD t(theta, 1.0);
  const SO2r<SD> Y = so2r_mul(SO2r<SD>{SD(X[0]), SD(X[1])}, SO2r<SD>{t_cos(t), t_sin(t)});   // exp = (cos, sin)
  return G[0] * Y.c.d + G[1] * Y.s.d;
}

// ---- BackwardMode.IMPLICIT: gradient of phi = w^T g of one cost, phi = - m(x, log_radius) s^2 q log(E), E = Z^-1 C,
//      q = w_j - w_i (edges: Ad(D^-1) = 1) | w_p (priors), x = (s log E)^2 ------------------------------------------------------
template <typename S>
__device__ __forceinline__ void so2_cost_phi(const SO2r<S>& Z, const SO2r<S>& C, double q, double s, S& phi, S& x, S& xi) {
  xi = so2r_log(so2r_mul(so2r_inv(Z), C));
  phi = S(0.0) - S(s * s) * S(q) * xi;
  x = S(s * s) * xi * xi;
}

// gZ: the 2 raw entries of Z; gs: the weight; glr: log_radius
__device__ __forceinline__ void so2_cost_vjp(const double* Z, const double* C, double q, double s, int loss, double log_radius,
                                             double* gZ, double* gs, double* glr) {
  double phi, x, xi, Phi;
  so2_cost_phi<double>(SO2r<double>{Z[0], Z[1]}, SO2r<double>{C[0], C[1]}, q, s, phi, x, xi);
  RobustTerms<1> rt;   // robust.cuh
  rt.eval(loss, &x, log_radius);
  rt.group(&phi, &Phi);
  *glr = phi * rt.m_l[0];
  *gs = rt.m[0] * (-2.0 * s * q * xi) + Phi * rt.m_x[0] * (2.0 * s * xi * xi);
  const SO2r<SD> Cd{SD(C[0]), SD(C[1])};
  for (int k = 0; k < 2; ++k) {   // one dual evaluation per raw entry [cos, sin] of Z
    SD phid, xd, xid;
    so2_cost_phi<SD>(so2r_seed(Z, k), Cd, q, s, phid, xd, xid);
    gZ[k] = rt.m[0] * phid.d + Phi * rt.m_x[0] * xd.d;
  }
}

// ---- BackwardMode.UNROLL / TRUNCATED: one cost's phi = -(J w) (r + J delta) [- lambda s^2 sum_i w_i delta_i J_i^2] (unroll_se3.cuh
//      states the maths) with J_j = s, J_i = -s (Between), J = s (Difference / Local prior: X = Xj, T = Z; Xi unused) ----------------
template <bool EDGE>
__device__ __forceinline__ void so2_unroll_phi(const SO2r<SD>& Xi, const SO2r<SD>& Xj, const SO2r<SD>& Z, double s, double wi,
                                               double wj, double di, double dj, double lam, SD& phi, SD& x, double* a_out,
                                               double* b_out, double* ell_out, double* xi_out) {
  const SO2r<SD> D = EDGE ? so2r_mul(so2r_inv(Xi), Xj) : Xj;
  const SD xi = so2r_log(so2r_mul(so2r_inv(Z), D));
  const double a = EDGE ? wj - wi : wj;   // Jlog (w_j - Ad(D^-1) w_i), Jlog = Ad = 1
  const double c = EDGE ? dj - di : dj;
  const SD bsum = xi + SD(c);
  phi = SD(0.0) - SD(s * s) * (SD(a) * bsum);
  x = SD(s * s) * (xi * xi);
  if (a_out) {
    *a_out = a;
    *b_out = bsum.v;
    *xi_out = xi.v;
  }
  // ellipsoidal damping: -lambda s^2 (J^2 w_j delta_j + (J Ad)^2 w_i delta_i), J^2 = (J Ad)^2 = 1
  const double ell = lam != 0.0 ? (EDGE ? wj * dj + wi * di : wj * dj) : 0.0;
  if (lam != 0.0) phi = phi - SD(lam * s * s) * SD(ell);
  if (ell_out) *ell_out = ell;
}

// g[0..2) w.r.t. Xi, [2..4) Xj (the prior's variable), [4..6) Z (the prior's target); gs (the weight); glr.  raw_*: 2 doubles each
// (raw_i unused for a prior; g[0..2) is then left alone)
template <bool EDGE>
__device__ __forceinline__ void so2_unroll_vjp(const double* raw_i, const double* raw_j, const double* raw_z, double s, double wi,
                                               double wj, double di, double dj, double lam, int loss, double log_radius, double* g,
                                               double* gs, double* glr) {
  SD phi, x;
  double a, b, ell, xi, P;
  so2_unroll_phi<EDGE>(so2r_seed(raw_i, -1), so2r_seed(raw_j, -1), so2r_seed(raw_z, -1), s, wi, wj, di, dj, lam, phi, x, &a, &b,
                       &ell, &xi);
  RobustTerms<1> rt;
  const double xv = x.v, pv = phi.v;
  rt.eval(loss, &xv, log_radius);
  rt.group(&pv, &P);
  *gs = rt.m[0] * (-2.0 * s * (a * b + lam * ell)) + P * rt.m_x[0] * (2.0 * s * xi * xi);
  *glr = pv * rt.m_l[0];
  for (int k = EDGE ? 0 : 2; k < 6; ++k) {   // one dual evaluation per raw entry
    const int which = k / 2, e = k % 2;
    so2_unroll_phi<EDGE>(so2r_seed(raw_i, which == 0 ? e : -1), so2r_seed(raw_j, which == 1 ? e : -1),
                         so2r_seed(raw_z, which == 2 ? e : -1), s, wi, wj, di, dj, lam, phi, x, nullptr, nullptr, nullptr, nullptr);
    g[k] = rt.m[0] * phi.d + P * rt.m_x[0] * x.d;
  }
}

}  // namespace thx
