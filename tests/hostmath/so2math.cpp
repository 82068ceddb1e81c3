// TEST-ONLY: the device maths of theseus_amd/csrc/vjp_so2.cuh compiled for the host (tests/test_so2_grad_host.py), over the same
// <hip/hip_runtime.h> shim as hostmath.cpp.
#include "vjp_so2.cuh"

using namespace thx;

extern "C" {

// out: gZ[2] gs[1] glr[1]
void so2_implicit_vjp(const double* Z, const double* C, double q, double s, int loss, double log_radius, double* out) {
  so2_cost_vjp(Z, C, q, s, loss, log_radius, out, out + 2, out + 3);
}

// out: g[6] (Xi, Xj, Z) gs[1] glr[1]; prior (edge = 0): the Xi pair stays 0, Xj = the variable, Z = the target
void so2_unroll(int edge, const double* Xi, const double* Xj, const double* Z, double s, double wi, double wj, double di, double dj,
                double lam, int loss, double log_radius, double* out) {
  if (edge) so2_unroll_vjp<true>(Xi, Xj, Z, s, wi, wj, di, dj, lam, loss, log_radius, out, out + 6, out + 7);
  else so2_unroll_vjp<false>(Xj, Xj, Z, s, wi, wj, di, dj, lam, loss, log_radius, out, out + 6, out + 7);
}

double so2_retract(const double* X, const double* G, double theta) { return so2_retract_vjp(X, G, theta); }
}
