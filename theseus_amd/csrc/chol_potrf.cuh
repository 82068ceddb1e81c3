#pragma once
#include "common.cuh"
#include "chol_base.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// blocked substitutions with a panel M in LDS (diag sub-blocks W_ss = L_ss^-1, below: -L_st)
// executed by wave 0 (64 lanes: lane = (row-in-block, half of the column range)); the caller
// brackets them with __syncthreads().  vec holds the right-hand side on entry, the solution on exit.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float half_sum(float x) { return x + __shfl_xor(x, 32); }
__device__ __forceinline__ double half_sum(double x) { return x + __shfl_xor(x, 32); }

// y = L_jj^-1 v :  for s: u_s = v_s + sum_{c < 32s} M[r][c] y[c] ;  y_s = W_ss u_s
template <typename T>
__device__ __forceinline__ void panel_forward(const T* M, T* vec, T* ubuf, int lane) {
  using C = CT<T>;
  const int rl = lane & 31, hf = lane >> 5;
#pragma unroll
  for (int sb = 0; sb < 4; ++sb) {
    const T* row = M + (32 * sb + rl) * C::LDM;
    T u = T(0);
    // columns [0, 32 sb) split between the two lane halves in 16-column slabs
    for (int c = 16 * hf; c < 32 * sb; c += 32)
#pragma unroll
      for (int i = 0; i < 16; ++i) u += row[c + i] * vec[c + i];
    u = half_sum(u) + vec[32 * sb + rl];
    if (hf == 0) ubuf[rl] = u;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
    T yv = T(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) yv += row[32 * sb + 16 * hf + i] * ubuf[16 * hf + i];
    yv = half_sum(yv);
    __builtin_amdgcn_wave_barrier();
    if (hf == 0) vec[32 * sb + rl] = yv;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
}

// x = L_jj^-T z :  for t = 3..0: a_t = z_t + sum_{r >= 32(t+1)} M[r][c] x[r] ;  x_t = W_tt^T a_t
template <typename T>
__device__ __forceinline__ void panel_backward(const T* M, T* vec, T* ubuf, int lane) {
  using C = CT<T>;
  const int cl = lane & 31, hf = lane >> 5;
#pragma unroll
  for (int tb = 3; tb >= 0; --tb) {
    const T* col = M + 32 * tb + cl;
    T a = T(0);
    for (int r = 32 * (tb + 1) + 16 * hf; r < TILE; r += 32)
#pragma unroll
      for (int i = 0; i < 16; ++i) a += col[(r + i) * C::LDM] * vec[r + i];
    a = half_sum(a) + vec[32 * tb + cl];
    if (hf == 0) ubuf[cl] = a;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    T xv = T(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) xv += col[(32 * tb + 16 * hf + i) * C::LDM] * ubuf[16 * hf + i];
    xv = half_sum(xv);
    __builtin_amdgcn_wave_barrier();
    if (hf == 0) vec[32 * tb + cl] = xv;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------------
// 32x32 in-wave kernels of the diagonal-tile factorisation.  Straight-line code is kept SMALL and is
// re-used by a run-time loop over the four sub-blocks: a fully unrolled 128-step factorisation is
// ~120 KB of instructions, streams through the 64 KB instruction cache once per workgroup and runs at
// L2 instruction-fetch latency (measured: 2700 cycles per 120-instruction step).
// ------------------------------------------------------------------------------------------------
// lane r (= lane & 31) holds row r: a[c] = S[r][c].  On exit a[c] = L[r][c] for c <= r (columns above the
// diagonal are garbage).  Broadcasts go through SGPRs (v_readlane), no LDS round trips.  Returns the
// 1-based index of the first non-positive pivot (0 = positive definite).
template <typename T, int N>
__device__ __forceinline__ int potrf_reg(T (&a)[N]) {
  int bad = 0;
  static_for<N>([&](auto ic) __attribute__((always_inline)) {
    constexpr int c = decltype(ic)::value;
    T d = bcast(a[c], c);
    if (!(d > T(0))) {
      if (bad == 0) bad = c + 1;
      d = T(1);
    }
    const T isq = t_rsqrt(d);
    a[c] *= isq;  // L[r][c]
    static_for<N - 1 - c>([&](auto iq) __attribute__((always_inline)) {
      constexpr int q = c + 1 + decltype(iq)::value;
      a[q] -= a[c] * bcast(a[c], q);  // S[r][q] -= L[r][c] L[q][c]
    });
  });
  return bad;
}

// the wave's own LDS writes become visible to its reads
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

// Dss: the 32 x LDB block in LDS (S_ss on entry, W_ss on exit); Lg: global address of L's element (first row of the
// sub-block, first column of the sub-block), rows_valid = number of the sub-block's rows inside the matrix.
// Returns the 1-based index (within the sub-block) of the first non-positive pivot, 0 if none.
// The inverse comes for FREE: lanes 0..31 hold the rows of S_ss, lanes 32..63 the rows of the identity, and the factorisation's
// column operations (column c scaled by 1/sqrt(pivot), column q -= column c * L[q][c]) run over all 64 lanes in the same
// instructions.  S -> L = S U with U = L^-T, so the identity becomes U: lane 32 + r ends with a[q] = U[r][q] = W[q][r], exact
// zeros for q < r -- column r of W = L^-1 without a second N^2 / 2 chain of dependent FMAs (the blocked 16 + 16 scheme it replaced
// was 7 us per tile slower, profiles/r6/ah_).  One wave issues in order, so the chain's cost is its instruction count: 32 steps of
// (pivot broadcast, rsqrt, scale) + 496 (readlane, fma) pairs.
template <typename T>
__device__ __forceinline__ int potrf_inv32(T* Dss, T* Lg, int64_t ld, int rows_valid, int lane) {
  using C = CT<T>;
  using V = typename C::V;
  constexpr int LDB = C::LDB;
  const int r = lane & 31;
  const bool upper = lane >= 32;
  T a[32];
  {
    const V* rp = reinterpret_cast<const V*>(Dss + r * LDB);
#pragma unroll
    for (int q = 0; q < 32 / C::VEC; ++q) {
      const V v = rp[q];
      if constexpr (sizeof(T) == 4) {
        a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
      } else {
        a[2 * q] = v.x; a[2 * q + 1] = v.y;
      }
    }
#pragma unroll
    for (int q = 0; q < 32; ++q) a[q] = upper ? (q == r ? T(1) : T(0)) : a[q];
  }
  __builtin_amdgcn_wave_barrier();   // (every lane has read its row before column r of W overwrites the block)
  const int bad = potrf_reg<T, 32>(a);
  if (!upper) {   // L_ss -> global memory: one 32-element row per lane, zeros above the diagonal
    if (r < rows_valid) {
      V* gp = reinterpret_cast<V*>(Lg + (int64_t)r * ld);
#pragma unroll
      for (int q = 0; q < 32 / C::VEC; ++q) {
        if constexpr (sizeof(T) == 4)
          gp[q] = make_float4(4 * q <= r ? a[4 * q] : 0.f, 4 * q + 1 <= r ? a[4 * q + 1] : 0.f, 4 * q + 2 <= r ? a[4 * q + 2] : 0.f,
                              4 * q + 3 <= r ? a[4 * q + 3] : 0.f);
        else
          gp[q] = make_double2(2 * q <= r ? a[2 * q] : 0.0, 2 * q + 1 <= r ? a[2 * q + 1] : 0.0);
      }
    }
  } else {        // W_ss -> the LDS block, row-major: W[q][r] (zero above the diagonal by construction)
#pragma unroll
    for (int q = 0; q < 32; ++q) Dss[q * LDB + r] = a[q];
  }
  return bad;
}

}  // namespace thx
