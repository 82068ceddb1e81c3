// Backward of SO2 pose graphs: the 1-dof twins of vjp2_kernels.hip (BackwardMode.IMPLICIT) and vjp_unroll3_kernels.hip (UNROLL /
// TRUNCATED), over the maths of vjp_so2.cuh (plain autograd through theseus/geometry/so2.py's closed forms, as dual numbers):
//   thx_so2_retract_vjp  : grad_delta = < grad_X_new , d/d delta [ X exp(step * delta) ] >
//   thx_pgso2_vjp        : grad_theta of phi = w^T g, per cost  phi = - m(x, log_radius) s^2 q log(E), E = Z^-1 C
//   thx_pgso2_unroll_vjp : per cost, the gradient of phi = -(J w) (r + J delta) [- lambda sum_i w_i delta_i H_ii]
// One lane per (cost, problem); double arithmetic whatever the storage type; per-cost outputs, no atomics (the host sums the pose
// gradients of the unrolled backward in a fixed order).
#include "common.cuh"
#include "vjp_so2.cuh"

namespace thx {

template <typename T>
__device__ __forceinline__ void so2_load_raw(const T* __restrict__ p, double* r) {
  r[0] = (double)p[0];
  r[1] = (double)p[1];
}

template <typename T>
__global__ void __launch_bounds__(64)
pgso2_vjp_kernel(thx_pg_structure s, thx_pg_data d, const T* __restrict__ wvec, int64_t ldw, T* __restrict__ g_meas,
                 T* __restrict__ g_wb, T* __restrict__ g_tgt, T* __restrict__ g_wp, T* __restrict__ g_lrb, T* __restrict__ g_lrp) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y;
  const int B = d.batch;
  if (b >= B) return;
  const T* poses = static_cast<const T*>(d.poses);
  const T* wv = wvec + (int64_t)b * ldw;
  double Z[2], C[2], q, sw, gZ[2], gs, glr = 0.0, lr = 0.0;
  int loss = THX_LOSS_NONE;
  T *outZ, *outS, *outL = nullptr;
  if (c < s.num_edges) {
    const int e = c, i = s.edge_i[e], j = s.edge_j[e];
    const int64_t mB = d.meas_bstride ? B : 1, wB = d.w_between_bstride ? B : 1;
    double Xi[2], Xj[2];
    so2_load_raw(poses + ((int64_t)i * B + b) * 2, Xi);
    so2_load_raw(poses + ((int64_t)j * B + b) * 2, Xj);
    so2_load_raw(static_cast<const T*>(d.meas) + ((int64_t)e * mB) * 2 + (int64_t)b * d.meas_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_between) + ((int64_t)e * wB) + (int64_t)b * d.w_between_bstride;
    const SO2r<double> D = so2r_mul(so2r_inv(SO2r<double>{Xi[0], Xi[1]}), SO2r<double>{Xj[0], Xj[1]});   // D = v0^-1 v1
    C[0] = D.c;
    C[1] = D.s;
    q = (double)wv[j] - (double)wv[i];   // w_j - Ad(D^-1) w_i, Ad = 1
    sw = (double)wp[0];
    outZ = g_meas + ((int64_t)e * B + b) * 2;
    outS = g_wb + (int64_t)e * B + b;
    loss = loss_code(d.robust_between, d.loss_between, e);
    if (loss) lr = load_log_radius<T>(d.log_radius_between, e, b, B, d.log_radius_between_bstride);
    if (d.robust_between) outL = g_lrb ? g_lrb + (int64_t)e * B + b : nullptr;   // (a plain cost of a mixed role: 0)
  } else {
    const int k = c - s.num_edges, p = s.prior_pose[k];
    const int64_t tB = d.prior_target_bstride ? B : 1, wB = d.w_prior_bstride ? B : 1;
    so2_load_raw(poses + ((int64_t)p * B + b) * 2, C);
    so2_load_raw(static_cast<const T*>(d.prior_target) + ((int64_t)k * tB) * 2 + (int64_t)b * d.prior_target_bstride, Z);
    const T* wp = static_cast<const T*>(d.w_prior) + ((int64_t)k * wB) + (int64_t)b * d.w_prior_bstride;
    q = (double)wv[p];
    sw = (double)wp[0];
    outZ = g_tgt + ((int64_t)k * B + b) * 2;
    outS = g_wp + (int64_t)k * B + b;
    loss = loss_code(d.robust_prior, d.loss_prior, k);
    if (loss) lr = load_log_radius<T>(d.log_radius_prior, k, b, B, d.log_radius_prior_bstride);
    if (d.robust_prior) outL = g_lrp ? g_lrp + (int64_t)k * B + b : nullptr;
  }
  so2_cost_vjp(Z, C, q, sw, loss, lr, gZ, &gs, &glr);
  if (outL) *outL = (T)glr;
  outZ[0] = (T)gZ[0];
  outZ[1] = (T)gZ[1];
  *outS = (T)gs;
}

template <typename T>
__global__ void __launch_bounds__(64)
so2_retract_vjp_kernel(const T* __restrict__ poses, const T* __restrict__ delta, int64_t ldd, T step, const T* __restrict__ gout,
                       T* __restrict__ gdelta, int64_t ldg, int P, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int p = blockIdx.y;
  if (b >= B) return;
  double X[2], G[2];
  so2_load_raw(poses + ((int64_t)p * B + b) * 2, X);
  so2_load_raw(gout + ((int64_t)p * B + b) * 2, G);
  const double theta = (double)(delta[(int64_t)b * ldd + p] * step);
  gdelta[(int64_t)b * ldg + p] = (T)(so2_retract_vjp(X, G, theta) * (double)step);
}

template <typename T>
__global__ void __launch_bounds__(64)
pgso2_unroll_vjp_kernel(thx_pg_structure s, thx_pg_data d, const T* __restrict__ wvec, int64_t ldw, const T* __restrict__ dvec,
                        int64_t ldd, const T* __restrict__ ell_damping, T* __restrict__ g_pose_i, T* __restrict__ g_pose_j,
                        T* __restrict__ g_meas, T* __restrict__ g_wb, T* __restrict__ g_pose_p, T* __restrict__ g_tgt,
                        T* __restrict__ g_wp, T* __restrict__ g_lrb, T* __restrict__ g_lrp) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y;
  const int B = d.batch;
  if (b >= B) return;
  const T* poses = static_cast<const T*>(d.poses);
  const T* wv = wvec + (int64_t)b * ldw;
  const T* dv = dvec + (int64_t)b * ldd;
  const double lam = ell_damping ? (double)ell_damping[b] : 0.0;
  double ri[2], rj[2], rz[2], g[6], gs, glr = 0.0;
  if (c < s.num_edges) {
    const int e = c, i = s.edge_i[e], j = s.edge_j[e];
    const int64_t mB = d.meas_bstride ? B : 1, wB = d.w_between_bstride ? B : 1;
    so2_load_raw(poses + ((int64_t)i * B + b) * 2, ri);
    so2_load_raw(poses + ((int64_t)j * B + b) * 2, rj);
    so2_load_raw(static_cast<const T*>(d.meas) + ((int64_t)e * mB) * 2 + (int64_t)b * d.meas_bstride, rz);
    const double sw = (double)static_cast<const T*>(d.w_between)[(int64_t)e * wB + (int64_t)b * d.w_between_bstride];
    const int loss = loss_code(d.robust_between, d.loss_between, e);
    const double lr = loss ? load_log_radius<T>(d.log_radius_between, e, b, B, d.log_radius_between_bstride) : 0.0;
    so2_unroll_vjp<true>(ri, rj, rz, sw, (double)wv[i], (double)wv[j], (double)dv[i], (double)dv[j], lam, loss, lr, g, &gs, &glr);
    T* oi = g_pose_i + ((int64_t)e * B + b) * 2;
    T* oj = g_pose_j + ((int64_t)e * B + b) * 2;
    T* oz = g_meas + ((int64_t)e * B + b) * 2;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      oi[k] = (T)g[k];
      oj[k] = (T)g[2 + k];
      oz[k] = (T)g[4 + k];
    }
    g_wb[(int64_t)e * B + b] = (T)gs;
    if (d.robust_between && g_lrb) g_lrb[(int64_t)e * B + b] = (T)glr;
  } else {
    const int k0 = c - s.num_edges, p = s.prior_pose[k0];
    const int64_t tB = d.prior_target_bstride ? B : 1, wB = d.w_prior_bstride ? B : 1;
    so2_load_raw(poses + ((int64_t)p * B + b) * 2, rj);
    so2_load_raw(static_cast<const T*>(d.prior_target) + ((int64_t)k0 * tB) * 2 + (int64_t)b * d.prior_target_bstride, rz);
    const double sw = (double)static_cast<const T*>(d.w_prior)[(int64_t)k0 * wB + (int64_t)b * d.w_prior_bstride];
    const int loss = loss_code(d.robust_prior, d.loss_prior, k0);
    const double lr = loss ? load_log_radius<T>(d.log_radius_prior, k0, b, B, d.log_radius_prior_bstride) : 0.0;
    so2_unroll_vjp<false>(rj, rj, rz, sw, 0.0, (double)wv[p], 0.0, (double)dv[p], lam, loss, lr, g, &gs, &glr);
    T* ox = g_pose_p + ((int64_t)k0 * B + b) * 2;
    T* ot = g_tgt + ((int64_t)k0 * B + b) * 2;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      ox[k] = (T)g[2 + k];
      ot[k] = (T)g[4 + k];
    }
    g_wp[(int64_t)k0 * B + b] = (T)gs;
    if (d.robust_prior && g_lrp) g_lrp[(int64_t)k0 * B + b] = (T)glr;
  }
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_pgso2_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, void* grad_meas,
                  void* grad_w_between, void* grad_prior_target, void* grad_w_prior, void* grad_log_radius_between,
                  void* grad_log_radius_prior, int dtype, void* stream) {
  if (!s || !d || !w) return fail("thx_pgso2_vjp: null argument");
  if (s->num_edges > 0 && (!grad_meas || !grad_w_between)) return fail("thx_pgso2_vjp: null edge gradient buffer");
  if (s->num_priors > 0 && (!grad_prior_target || !grad_w_prior)) return fail("thx_pgso2_vjp: null prior gradient buffer");
  if (ldw < (int64_t)s->num_poses) return fail("thx_pgso2_vjp: ldw < n");
  if (const char* why = check_robust(d)) return fail(why);
  dim3 grid((d->batch + 63) / 64, s->num_edges + s->num_priors), block(64);
  if (grid.y == 0) return 0;
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(pgso2_vjp_kernel<float>, grid, block, 0, as_stream(stream), *s, *d, (const float*)w, ldw,
                                  (float*)grad_meas, (float*)grad_w_between, (float*)grad_prior_target, (float*)grad_w_prior,
                                  (float*)grad_log_radius_between, (float*)grad_log_radius_prior),
               hipLaunchKernelGGL(pgso2_vjp_kernel<double>, grid, block, 0, as_stream(stream), *s, *d, (const double*)w, ldw,
                                  (double*)grad_meas, (double*)grad_w_between, (double*)grad_prior_target,
                                  (double*)grad_w_prior, (double*)grad_log_radius_between, (double*)grad_log_radius_prior));
  return check_launch("thx_pgso2_vjp");
}

int thx_so2_retract_vjp(const void* poses, const void* delta, int64_t ldd, double step, const void* grad_out, void* grad_delta,
                        int64_t ldg, int32_t P, int32_t B, int dtype, void* stream) {
  if (!poses || !delta || !grad_out || !grad_delta || P <= 0 || B <= 0) return fail("bad so2_retract_vjp args");
  dim3 grid((B + 63) / 64, P), block(64);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(so2_retract_vjp_kernel<float>, grid, block, 0, as_stream(stream), (const float*)poses,
                                  (const float*)delta, ldd, (float)step, (const float*)grad_out, (float*)grad_delta, ldg, P, B),
               hipLaunchKernelGGL(so2_retract_vjp_kernel<double>, grid, block, 0, as_stream(stream), (const double*)poses,
                                  (const double*)delta, ldd, step, (const double*)grad_out, (double*)grad_delta, ldg, P, B));
  return check_launch("thx_so2_retract_vjp");
}

int thx_pgso2_unroll_vjp(const thx_pg_structure* s, const thx_pg_data* d, const void* w, int64_t ldw, const void* delta, int64_t ldd,
                         const void* ellipsoidal_damping, void* grad_pose_i, void* grad_pose_j, void* grad_meas,
                         void* grad_w_between, void* grad_pose_prior, void* grad_prior_target, void* grad_w_prior,
                         void* grad_log_radius_between, void* grad_log_radius_prior, int dtype, void* stream) {
  if (!s || !d || !w || !delta) return fail("thx_pgso2_unroll_vjp: null argument");
  if (s->num_edges > 0 && (!grad_pose_i || !grad_pose_j || !grad_meas || !grad_w_between))
    return fail("thx_pgso2_unroll_vjp: null edge gradient buffer");
  if (s->num_priors > 0 && (!grad_pose_prior || !grad_prior_target || !grad_w_prior))
    return fail("thx_pgso2_unroll_vjp: null prior gradient buffer");
  if (ldw < (int64_t)s->num_poses || ldd < (int64_t)s->num_poses) return fail("thx_pgso2_unroll_vjp: ldw / ldd < n");
  if (const char* why = check_robust(d)) return fail(why);
  dim3 grid((d->batch + 63) / 64, s->num_edges + s->num_priors), block(64);
  if (grid.y == 0) return 0;
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(pgso2_unroll_vjp_kernel<float>, grid, block, 0, as_stream(stream), *s, *d, (const float*)w, ldw,
                                  (const float*)delta, ldd, (const float*)ellipsoidal_damping, (float*)grad_pose_i,
                                  (float*)grad_pose_j, (float*)grad_meas, (float*)grad_w_between, (float*)grad_pose_prior,
                                  (float*)grad_prior_target, (float*)grad_w_prior, (float*)grad_log_radius_between,
                                  (float*)grad_log_radius_prior),
               hipLaunchKernelGGL(pgso2_unroll_vjp_kernel<double>, grid, block, 0, as_stream(stream), *s, *d, (const double*)w,
                                  ldw, (const double*)delta, ldd, (const double*)ellipsoidal_damping, (double*)grad_pose_i,
                                  (double*)grad_pose_j, (double*)grad_meas, (double*)grad_w_between, (double*)grad_pose_prior,
                                  (double*)grad_prior_target, (double*)grad_w_prior, (double*)grad_log_radius_between,
                                  (double*)grad_log_radius_prior));
  return check_launch("thx_pgso2_unroll_vjp");
}

}  // extern "C"
