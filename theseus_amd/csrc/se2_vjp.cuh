// What the stage A kernels of the SE2 families' implicit backward (push_vjp_kernels.hip: thx_push2_vjp, trajse2_vjp_kernels.hip:
// thx_trajse2_vjp) share: the fp64 / Dual<double> forms of an SE2 record with the forward's Taylor branch forced, and the backward of
// a Difference on SE2 (records go out through RecOutT of term_family.cuh).  Included after the source's own
// ``#pragma clang fp contract(off)``.
#pragma once
#include <cmath>

#include "term_family.cuh"
#include "lie_se2.cuh"
#include "dual.cuh"

namespace thx {

using D64 = Dual<double>;

template <typename T>
__device__ __forceinline__ SE2<double> widen(const SE2<T>& X) {
  return SE2<double>{(double)X.x, (double)X.y, (double)X.c, (double)X.s};
}
// SE2<Dual>: X with the unit tangent on raw component k (k < 0: a constant)
__device__ __forceinline__ SE2<D64> seeded(const SE2<double>& X, int k) {
  return SE2<D64>{D64(X.x, k == 0 ? 1.0 : 0.0), D64(X.y, k == 1 ? 1.0 : 0.0), D64(X.c, k == 2 ? 1.0 : 0.0),
                  D64(X.s, k == 3 ? 1.0 : 0.0)};
}
// thresholds that make the fp64 / Dual<double> helpers take the branches the forward took in the run's dtype
template <typename S = D64>
__device__ __forceinline__ Eps2<S> forced(bool small, bool dsmall) {
  return Eps2<S>{S(small ? HUGE_VAL : 0.0), S(dsmall ? HUGE_VAL : 0.0)};
}
// the cotangent's three columns of state variable ``var``
template <typename T>
__device__ __forceinline__ void load_u(const T* __restrict__ ub, int var, double* o) {
  o[0] = (double)ub[3 * var], o[1] = (double)ub[3 * var + 1], o[2] = (double)ub[3 * var + 2];
}

// Difference on SE2 with row weights w and the variable's cotangent uu; record: 0-3 target (raw x, y, cos, sin), 4-6 weight
template <typename T, typename Out>
__device__ __forceinline__ void se2_prior_vjp(const SE2<T>& target_t, const SE2<T>& var_t, const double* w, const double* uu, int wdim,
                                              const Eps2<T>& eps, const Out& out) {
  // the forward's Taylor decisions (local_eval2, se2_log_jlog), in the run's dtype
  bool small, dsmall;
  {
    SE2<T> ti, D;
    se2_inv(target_t, ti);
    se2_mul(ti, var_t, D);
    const T th = t_abs(t_atan2(D.s, D.c));
    small = th < eps.nz, dsmall = th < eps.dnz;
  }
  const SE2<double> target = widen(target_t);
  const SE2<D64> var = seeded(widen(var_t), -1);
  const Eps2<D64> branch = forced(small, dsmall);
  double gw[3] = {0.0, 0.0, 0.0};
  // both the error and the block (Jlog) depend on the target: phi = -sum_i w_i^2 (Jlog u)_i xi_i
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    SE2<D64> ti, D;
    D64 xi[3], Jl[9];
    se2_inv(seeded(target, k), ti);
    se2_mul(ti, var, D);
    se2_log_jlog<D64>(D, branch, xi, Jl, true);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const D64 q = (Jl[3 * i] * D64(uu[0]) + Jl[3 * i + 1] * D64(uu[1]) + Jl[3 * i + 2] * D64(uu[2])) * xi[i];
      acc += w[i] * w[i] * q.d;
      gw[i] = -2.0 * w[i] * q.v;
    }
    out.put(k, -acc);
  }
  out.weights(4, wdim, gw);
}

}  // namespace thx
