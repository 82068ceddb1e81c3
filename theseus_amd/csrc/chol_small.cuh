#pragma once
#include "common.cuh"
#include "chol_tiles.cuh"
#include "chol_solve.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// small helpers: diagonal extraction, LM accept test
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void diag_kernel(const T* __restrict__ H, int64_t ld, int n, T* __restrict__ d, int64_t ldv) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[(int64_t)b * ldv + i] = H[(int64_t)b * ld * ld + (int64_t)i * ld + i];
}

template <typename T>
__global__ void __launch_bounds__(64)
lm_accept_kernel(const T* __restrict__ delta, const T* __restrict__ g, int64_t ldv, const T* __restrict__ H,
                 int64_t ld, int n, T* __restrict__ damping, const T* __restrict__ prev_err,
                 const T* __restrict__ new_err, int ellipsoidal, T accept, T down, T up, uint8_t* __restrict__ reject) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const T lam = damping[b];
  T s = T(0);
  for (int i = lane; i < n; i += 64) {
    const T dl = delta[(int64_t)b * ldv + i];
    const T D = ellipsoidal ? H[(int64_t)b * ld * ld + (int64_t)i * ld + i] * lam : lam;
    s += dl * (D * dl + g[(int64_t)b * ldv + i]);
  }
  s = wave_sum(s);
  if (lane == 0) {
    const T den = s / T(2);
    const T rho = (prev_err[b] - new_err[b]) / den;
    const bool rej = rho <= accept;
    T nl = rej ? lam * up : lam / down;
    nl = nl < T(1.0e-7) ? T(1.0e-7) : (nl > T(1.0e7) ? T(1.0e7) : nl);
    damping[b] = nl;
    reject[b] = rej ? 1 : 0;
  }
}

// right-looking schedule: the damping of the diagonal elements d >= d0 of the working matrix in the L frame,
// A_dd += ellipsoidal ? lambda H_dd + eps : lambda, with H_dd the ORIGINAL diagonal (dense H frame or block list) -- block column 0
// gets its damping from chol_diag as always; the other diagonal tiles have just been written by the first trailing update
template <typename T>
__global__ void rl_damp_kernel(T* __restrict__ L, int64_t ld, const T* __restrict__ H, int64_t ldh, HBlk hb,
                               const T* __restrict__ damping, int ellipsoidal, T eps, int d0, int n) {
  const int b = blockIdx.y, d = d0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  const T lam = damping[b];
  T add = lam;
  if (ellipsoidal) {
    T h;
    if (hb.blocks) {
      const int v = d / hb.bd, e = d % hb.bd;
      h = static_cast<const T*>(hb.blocks)[(int64_t)b * hb.bstride + (int64_t)hb.diag_blk[v] * hb.bd * hb.bd + e * hb.bd + e];
    } else {
      h = H[(int64_t)b * ldh * ldh + (int64_t)d * ldh + d];
    }
    add = lam * h + eps;
  }
  L[(int64_t)b * ld * ld + (int64_t)d * ld + d] += add;
}

// dst[b][k] = idx[k] >= 0 ? src[b][idx[k]] : 0  -- the solver's permuted / padded vectors <-> the linearization's (thx_vec_gather)
template <typename T>
__global__ void vec_gather_kernel(const T* __restrict__ src, int64_t lds, T* __restrict__ dst, int64_t ldd,
                                  const int32_t* __restrict__ idx, int n) {
  const int b = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int i = idx[k];
  dst[(int64_t)b * ldd + k] = i >= 0 ? src[(int64_t)b * lds + i] : T(0);
}

}  // namespace thx
