// The backward of the planar-pushing implicit step (thx_push2_vjp): with g = -sum_t J_t^T e_t what thx_push2_eval +
// thx_block_assemble form at a detached state and u a cotangent of g, the gradient of u^T g w.r.t. the auxiliary tensors -- what
// autograd computes by walking the torch classes of theseus_amd/embodied.py and se2_torch.py back.  Per term
//   phi_t = -(sum_s J_s u_s) . e_t = -sum_i w_i^2 c_i e_i,   c = sum_s J_s^raw u_s,  e the raw error, w the row weights.
//
// Stage A (push2_vjp_terms_kernel): one thread per (term, problem), problems fastest, push2_eval_kernel's map and guards.  A thread
// stores each entry of its THX_PUSH2_REC-double record as soon as it has it (the stores of a wave are consecutive doubles), so no
// record lives in registers or scratch.  Every branch of the forward -- the in-grid test, floor, d < r, the Taylor switches of the
// SE2 log -- is decided in the run's dtype by the forward's own operations (push_family.cuh, lie_se2.cuh, sdf_bilinear_cells; the
// pragma below covers them); the derivatives are fp64:
//   QuasiStaticPushingPlanar     closed forms: c is the directional derivative of D V - Vp along u, c_square enters e_2 and c_2 only
//   MovingFrameBetween           c from the chain of the three betweens; d log(meas^-1 D) / d meas by the SE2 helpers on
//                                Dual<double>, one pass per raw component (x, y, cos, sin), the Taylor branch forced to the forward's
//   Difference on SE2            the same passes through the error AND the block (Jlog depends on the target): se2_vjp.cuh
//   EffectorObjectContactPlanar  phi = -w^2 sgn s |d - r|, s = (j1, j2) . (G u_obj + H u_eff): collision_vjp's structure
//                                (traj_kernels.hip) with the gap |d - r|; sgn and sign(d - r) are constants, as in the torch class
// Stage B: vjp_reduce_kernel, vjp_scatter_kernel and vjp_grid_out_kernel of term_family.cuh on the records.  No atomics.
#pragma clang fp contract(off)
#include "push_family.cuh"
#include "se2_vjp.cuh"

namespace thx {

constexpr int kRec = THX_PUSH2_REC;
using RecOut = RecOutT<kRec>;   // (RecOutT, widen, seeded, forced, load_u: se2_vjp.cuh)

template <typename T>
__device__ __forceinline__ void row_weights64(const thx_push2_term& tm, int k, int b, double* w) {
  T wt[3];
  row_weights<T>(tm, k, b, wt);
  w[0] = (double)wt[0], w[1] = (double)wt[1], w[2] = (double)wt[2];
}

// record: 0 c_square, 1-3 weight
template <typename T>
__device__ __forceinline__ void qsp_vjp(const thx_push2_term& tm, const SE2<double>& o1, const SE2<double>& o2, const SE2<double>& e1,
                                        const SE2<double>& e2, const T* __restrict__ ub, int b, const RecOut& out) {
  const double c2 = (double)aux_at<T>(tm, 0, b);
  double w[3], u1[3], u2[3], u3[3], u4[3];
  row_weights64<T>(tm, 1, b, w);
  load_u(ub, tm.pose[0], u1), load_u(ub, tm.pose[1], u2), load_u(ub, tm.pose[2], u3), load_u(ub, tm.pose[3], u4);
  // qsp_term's quantities
  double px, py, vx, vy, qx, qy;
  unrotate(o2.c, o2.s, e2.x - o2.x, e2.y - o2.y, px, py);
  unrotate(o2.c, o2.s, o2.x - o1.x, o2.y - o1.y, vx, vy);
  unrotate(o2.c, o2.s, e2.x - e1.x, e2.y - e1.y, qx, qy);
  SE2<double> o1i, od;
  se2_inv(o1, o1i);
  se2_mul(o1i, o2, od);
  const double om = atan2(od.s, od.c);
  const double e[3] = {vx - py * om - qx, vy + px * om - qy, -py * vx + px * vy - c2 * om};
  // their derivatives along u: a pose's translation moves by R(X) u_xy, its angle by u_theta; R2^T R(X) u_xy =
  double a1x, a1y, a2x, a2y, b1x, b1y, b2x, b2y;
  auto rtr = [&](const SE2<double>& X, const double* uu, double& rx, double& ry) {
    unrotate(o2.c, o2.s, X.c * uu[0] - X.s * uu[1], X.s * uu[0] + X.c * uu[1], rx, ry);
  };
  rtr(o1, u1, a1x, a1y), rtr(o2, u2, a2x, a2y), rtr(e1, u3, b1x, b1y), rtr(e2, u4, b2x, b2y);
  const double dvx = a2x - a1x + vy * u2[2], dvy = a2y - a1y - vx * u2[2], dom = u2[2] - u1[2];
  const double dpx = b2x - u2[0] + py * u2[2], dpy = b2y - u2[1] - px * u2[2];   // (transform_to's own -1: no R2^T R2 here)
  const double dqx = b2x - b1x + qy * u2[2], dqy = b2y - b1y - qx * u2[2];
  const double c[3] = {-dpy * om + dvx - py * dom - dqx, dpx * om + dvy + px * dom - dqy,
                       (-dpy * vx + dpx * vy) + (-py * dvx + px * dvy - c2 * dom)};
  // c_square enters e_2 (-om) and c_2 (-dom)
  out.put(0, w[2] * w[2] * (dom * e[2] + c[2] * om));
  const double gw[3] = {-2.0 * w[0] * c[0] * e[0], -2.0 * w[1] * c[1] * e[1], -2.0 * w[2] * c[2] * e[2]};
  out.weights(1, tm.wdim, gw);
  out.zeros(4);
}

// record: 0-3 measurement (raw x, y, cos, sin), 4-6 weight
template <typename T>
__device__ __forceinline__ void mfb_vjp(const thx_push2_term& tm, const SE2<T>& f1t, const SE2<T>& f2t, const SE2<T>& p1t,
                                        const SE2<T>& p2t, const T* __restrict__ ub, int b, const Eps2<T>& eps, const RecOut& out) {
  const SE2<T> meas_t = aux_pose<T>(tm, 0, b);
  // the forward's Taylor decision (mfb_term, se2_log_jlog), in the run's dtype
  bool small;
  {
    SE2<T> p1f, p2f, vd, mi, E;
    between_j0<T>(f1t, p1t, p1f, nullptr, false);
    between_j0<T>(f2t, p2t, p2f, nullptr, false);
    between_j0<T>(p1f, p2f, vd, nullptr, false);
    se2_inv(meas_t, mi);
    se2_mul(mi, vd, E);
    small = t_abs(t_atan2(E.s, E.c)) < eps.nz;
  }
  double w[3], u1[3], u2[3], u3[3], u4[3];
  row_weights64<T>(tm, 1, b, w);
  load_u(ub, tm.pose[0], u1), load_u(ub, tm.pose[1], u2), load_u(ub, tm.pose[2], u3), load_u(ub, tm.pose[3], u4);
  SE2<double> p1f, p2f, vd;
  double JB1[9], JB2[9], JO1[9], Jf1[9], cr[3], cw[3];
  between_j0(widen(f1t), widen(p1t), p1f, JB1, true);
  between_j0(widen(f2t), widen(p2t), p2f, JB2, true);
  between_j0(p1f, p2f, vd, JO1, true);
  mat3_mul(JO1, JB1, Jf1);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double c = u4[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) c += Jf1[3 * i + d] * u1[d] + JB2[3 * i + d] * u2[d] + JO1[3 * i + d] * u3[d];
    cr[i] = c, cw[i] = c * w[i] * w[i];
  }
  // the blocks do not depend on the measurement: d phi / d meas_k = -(c w^2) . d log(meas^-1 vd) / d meas_k
  const SE2<double> meas = widen(meas_t);
  const SE2<D64> vdd = seeded(vd, -1);
  const Eps2<D64> branch = forced(small, small);
  double xi0[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    SE2<D64> mi, E;
    D64 xi[3];
    se2_inv(seeded(meas, k), mi);
    se2_mul(mi, vdd, E);
    se2_log_jlog<D64>(E, branch, xi, nullptr, false);
    out.put(k, -(cw[0] * xi[0].d + cw[1] * xi[1].d + cw[2] * xi[2].d));
    xi0[0] = xi[0].v, xi0[1] = xi[1].v, xi0[2] = xi[2].v;
  }
  const double gw[3] = {-2.0 * w[0] * cr[0] * xi0[0], -2.0 * w[1] * cr[1] * xi0[1], -2.0 * w[2] * cr[2] * xi0[2]};
  out.weights(4, tm.wdim, gw);
  out.zeros(7);
}

// record: 0-3 target (raw x, y, cos, sin), 4-6 weight: se2_prior_vjp of se2_vjp.cuh, through both the error and the block
template <typename T>
__device__ __forceinline__ void prior_vjp(const thx_push2_term& tm, const SE2<T>& var_t, const T* __restrict__ ub, int b,
                                          const Eps2<T>& eps, const RecOut& out) {
  double w[3], uu[3];
  row_weights64<T>(tm, 1, b, w);
  load_u(ub, tm.pose[0], uu);
  se2_prior_vjp<T>(aux_pose<T>(tm, 0, b), var_t, w, uu, tm.wdim, eps, out);
  out.zeros(7);
}

// record (collision_vjp's layout): 0-3 d / d corner value (ll, hl, lh, hh), 4-7 their cell indices row * cols + col, 8-9 origin,
// 10 cell size, 11 effector radius, 12 weight; all zero outside the grid, where the error and the blocks are constants
template <typename T>
__device__ __forceinline__ void contact_vjp(const thx_push2_term& tm, const SE2<T>& obj, const SE2<T>& eff, const T* __restrict__ ub,
                                            int b, const RecOut& out) {
  const T* sdf = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T ox_t = aux_at<T>(tm, 1, b, 0), oy_t = aux_at<T>(tm, 1, b, 1), cell_t = aux_at<T>(tm, 2, b), rad_t = aux_at<T>(tm, 3, b);
  // contact_term's geometry, in the run's dtype
  T px_t, py_t, dist, j1, j2;
  SdfCells<T> k;
  unrotate(obj.c, obj.s, eff.x - obj.x, eff.y - obj.y, px_t, py_t);
  sdf_bilinear_cells<T>(sdf, tm.rows, tm.cols, ox_t, oy_t, cell_t, px_t, py_t, dist, j1, j2, k);
  if (k.oob) {
    out.zeros(0);
    return;
  }
  const T diff = dist - rad_t;
  const double sgn = dist < rad_t ? -1.0 : 1.0;                              // the Jacobians' sign (eff_obj_contact.py)
  const double sg = diff > (T)0 ? 1.0 : (diff < (T)0 ? -1.0 : 0.0);          // d |d - r| / d d, as torch's abs() returns it
  // ... and in fp64 from the same state
  const SE2<double> O = widen(obj), E = widen(eff);
  double px, py, uo[3], ue[3];
  unrotate(O.c, O.s, E.x - O.x, E.y - O.y, px, py);
  load_u(ub, tm.pose[0], uo), load_u(ub, tm.pose[1], ue);
  // v = G u_obj + H u_eff: G = [[-1, 0, py], [0, -1, -px]], H = R(obj)^T [R(eff) | 0]
  double hx, hy;
  unrotate(O.c, O.s, E.c * ue[0] - E.s * ue[1], E.s * ue[0] + E.c * ue[1], hx, hy);
  const double vx = -uo[0] + py * uo[2] + hx, vy = -uo[1] - px * uo[2] + hy;
  const double w = (double)aux_at<T>(tm, 4, b), rad = (double)rad_t, cell = (double)cell_t, w2 = w * w;
  const double col = (px - (double)ox_t) / cell, row = (py - (double)oy_t) / cell;
  const double lr = (double)k.lr, lc = (double)k.lc;
  const double hrd = lr + 1.0 - row, hcd = lc + 1.0 - col, lrd = row - lr, lcd = col - lc;
  const double sll = (double)k.sll, shl = (double)k.shl, slh = (double)k.slh, shh = (double)k.shh;
  const double d = hrd * hcd * sll + lrd * hcd * shl + hrd * lcd * slh + lrd * lcd * shh;
  const double dc = hrd * (slh - sll) + lrd * (shh - shl), dr = hcd * (shl - sll) + lcd * (shh - slh);   // d d / d col, d d / d row
  const double s = (dc * vx + dr * vy) / cell;
  // phi = -w^2 sgn s |d - r|:  d phi = A ds + S dd - S dr
  const double A1 = -sgn * sg * (d - rad), A = w2 * A1, S = -w2 * sgn * sg * s;
  out.put(0, A * (-hrd * vx - hcd * vy) / cell + S * hrd * hcd);
  out.put(1, A * (-lrd * vx + hcd * vy) / cell + S * lrd * hcd);
  out.put(2, A * (hrd * vx - lcd * vy) / cell + S * hrd * lcd);
  out.put(3, A * (lrd * vx + lcd * vy) / cell + S * lrd * lcd);
  out.put(4, (double)((int64_t)k.lri * tm.cols + k.lci));
  out.put(5, (double)((int64_t)k.hri * tm.cols + k.lci));
  out.put(6, (double)((int64_t)k.lri * tm.cols + k.hci));
  out.put(7, (double)((int64_t)k.hri * tm.cols + k.hci));
  // through col = (px - ox) / cell, row = (py - oy) / cell; the only second derivative of the bilinear form is the mixed one
  const double mixed = sll - shl - slh + shh;
  const double pcol = A * mixed * vy / cell + S * dc, prow = A * mixed * vx / cell + S * dr;
  out.put(8, -pcol / cell);
  out.put(9, -prow / cell);
  out.put(10, -(pcol * col + prow * row + A * s) / cell);   // (the last: j1, j2 divide by the cell size themselves)
  out.put(11, -S);
  out.put(12, 2.0 * w * A1 * s);
  out.zeros(13);
}

// stage A: push2_eval_kernel's map and guards; every (term, problem) writes its whole record, zeros where the term is skipped
template <typename T>
__global__ void __launch_bounds__(256)
push2_vjp_terms_kernel(const thx_push2_term* __restrict__ terms, int n_terms, const T* __restrict__ x, int V,
                       const T* __restrict__ u, int64_t ldu, int m, int64_t j_total, double* __restrict__ rec, int B, Eps2<T> eps) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_push2_term& tm = terms[t];   // (read in place, as the forward does)
  const RecOut out{rec + (int64_t)t * kRec * B + b, (int64_t)B};
  if (!push_reads_ok(tm, V) || !push_writes_ok(tm, m, j_total)) {
    out.zeros(0);
    return;
  }
  const T* ub = u + (int64_t)b * ldu;
  const SE2<T> a = load_pose(x, (int64_t)tm.pose[0] * B + b);
  if (tm.kind == THX_PUSH2_PRIOR) {
    prior_vjp<T>(tm, a, ub, b, eps, out);
    return;
  }
  const SE2<T> c = load_pose(x, (int64_t)tm.pose[1] * B + b);
  if (tm.kind == THX_PUSH2_CONTACT) {
    contact_vjp<T>(tm, a, c, ub, b, out);
    return;
  }
  const SE2<T> d = load_pose(x, (int64_t)tm.pose[2] * B + b);
  const SE2<T> f = load_pose(x, (int64_t)tm.pose[3] * B + b);
  if (tm.kind == THX_PUSH2_QSP)
    qsp_vjp<T>(tm, widen(a), widen(c), widen(d), widen(f), ub, b, out);
  else
    mfb_vjp<T>(tm, a, c, d, f, ub, b, eps, out);
}

}  // namespace thx

using namespace thx;

extern "C" int thx_push2_vjp(const thx_push2_term* terms, int32_t n_terms, const void* x, int32_t V, const void* u, int64_t ldu,
                             int32_t m, int64_t j_total, double* rec, const thx_traj2_grad_plan* plan, void* grad_out,
                             double* grid_work, int32_t B, int dtype, const thx_se2_eps* eps, void* stream) {
  const char* who = "thx_push2_vjp";
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
               hipLaunchKernelGGL(push2_vjp_terms_kernel<float>, dim3(term_blocks), block, 0, s, terms, n_terms, (const float*)x, V,
                                  (const float*)u, ldu, m, j_total, rec, B, make_eps2<float>(eps)),
               hipLaunchKernelGGL(push2_vjp_terms_kernel<double>, dim3(term_blocks), block, 0, s, terms, n_terms, (const double*)x, V,
                                  (const double*)u, ldu, m, j_total, rec, B, make_eps2<double>(eps)));
  if (int rc = family_vjp_stage_b<thx_push2_term, THX_PUSH2_CONTACT, kRec>(rec, terms, n_terms, p, grad_out, grid_work, B, dtype, s))
    return rc;
  return check_launch(who);
}
