// Batched dense LU with partial (row) pivoting, P M = L U, for gfx950 -- the HIP counterpart of the reference's
// LUDenseSolver (theseus/optimizer/linear/dense_solver.py:125-141: torch.linalg.lu_factor + lu_solve on AtA + damping).
//
// One independent n x n system per batch item, fp32 / fp64, in the dense row-major (B, ld, ld) frames of the Cholesky
// (ld % 32 == 0).  Right-looking, blocked by NB = 32 columns.  Per block column k0:
//   lu_panel_kernel      one 1024-thread workgroup per problem: rows k0..n-1 of the 32 panel columns, eight columns at a
//                        time in registers (a thread owns up to four rows).  Per column: workgroup-wide arg-max of |value|
//                        (ties -> lowest row, LAPACK's i?amax), row interchange, scaling, update of the register columns;
//                        after each eight columns an 8 x rem unit-lower solve and a rank-8 update of the panel's
//                        remaining columns.  Writes piv (getrf convention, 0-based) and info (first exactly zero pivot + 1).
//   lu_swap_trsm_kernel  one wave per (problem, 32-column block outside the panel): the panel's 32 row interchanges on
//                        that block; right of the panel also U12 = L11^-1 A12 on the matrix cores -- X = L11^-1 (unit
//                        lower, registers), U = X A, one refinement step U += X (A - L11 U), so that U12 has the
//                        residual of a substitution and not that of a product with an explicit inverse.
//   lu_trailing_kernel   A22 -= L21 U12 on the matrix cores, one 128 x 64 tile per four-wave workgroup, both operands
//                        staged through LDS (K = 32).
// Rows / columns n..ld-1 of the working frame are identity padding written by lu_load_kernel, which also writes every
// other element of the frame: nothing depends on what LU, piv or info held before.  The source matrix is only read.
//
// Limits: n <= LU_MAX_N = 4096 (a panel thread owns at most four rows; the solves keep the vector, one diagonal block
// and the pivots in 57 KB of LDS in fp64), refused on the host before any launch.
#include "common.cuh"

namespace thx {

constexpr int NB = 32;            // panel width / block edge
constexpr int LU_MAX_N = 4096;    // see above
constexpr int PANEL_NT = 1024;    // threads of the panel workgroup
constexpr int PANEL_ROWS = LU_MAX_N / PANEL_NT;   // rows a panel thread owns at most
constexpr int SUBW = 8;           // panel columns held in registers at a time
constexpr int BLS = NB + 1;       // LDS row stride of a 32 x 32 block

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// One wave's 32 x 32 block product on the matrix cores: D += sign * A B, A row major [i][k] with stride lsa, B row major
// [k][j] with stride lsb, both in LDS.  A lane holds 16 elements of D; element e sits at (row(e, lane), col(e, lane)).
template <typename T>
struct Mma;

template <>
struct Mma<float> {   // v_mfma_f32_32x32x2_f32: lane (i = l & 31, k = l >> 5) of A, (k, j = l & 31) of B
  using Frag = f32x16;
  static __device__ __forceinline__ int row(int e, int l) { return 8 * (e >> 2) + 4 * (l >> 5) + (e & 3); }
  static __device__ __forceinline__ int col(int, int l) { return l & 31; }
  static __device__ __forceinline__ float get(const Frag& d, int e) { return d[e]; }
  static __device__ __forceinline__ void set(Frag& d, int e, float x) { d[e] = x; }
  static __device__ __forceinline__ void mac(Frag& d, const float* sA, int lsa, const float* sB, int lsb, float sign, int l) {
    const int i = l & 31, g = l >> 5;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 2 * kk + g;
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(sign * sA[i * lsa + k], sB[k * lsb + i], d, 0, 0, 0);
    }
  }
};

template <>
struct Mma<double> {   // v_mfma_f64_16x16x4_f64, four 16 x 16 blocks: lane (i = l & 15, k = l >> 4) of A, (k, j = l & 15) of B
  struct Frag {
    f64x4 v[4];   // block (ih, jh) = v[2 ih + jh]
  };
  static __device__ __forceinline__ int row(int e, int l) { return 16 * (e >> 3) + 4 * (e & 3) + (l >> 4); }
  static __device__ __forceinline__ int col(int e, int l) { return 16 * ((e >> 2) & 1) + (l & 15); }
  static __device__ __forceinline__ double get(const Frag& d, int e) { return d.v[e >> 2][e & 3]; }
  static __device__ __forceinline__ void set(Frag& d, int e, double x) { d.v[e >> 2][e & 3] = x; }
  static __device__ __forceinline__ void mac(Frag& d, const double* sA, int lsa, const double* sB, int lsb, double sign, int l) {
    const int i = l & 15, g = l >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + g;
      const double a0 = sign * sA[i * lsa + k], a1 = sign * sA[(16 + i) * lsa + k];
      const double b0 = sB[k * lsb + i], b1 = sB[k * lsb + 16 + i];
      d.v[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, d.v[0], 0, 0, 0);
      d.v[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, d.v[1], 0, 0, 0);
      d.v[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, d.v[2], 0, 0, 0);
      d.v[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d.v[3], 0, 0, 0);
    }
  }
};

template <typename T>
__device__ __forceinline__ T absval(T x) {
  return x < T(0) ? -x : x;
}

// (|value|, row) of a pivot candidate beats another: larger magnitude, ties to the lower row (LAPACK i?amax)
template <typename T>
__device__ __forceinline__ bool pivot_beats(T oa, int oi, T ba, int bi) {
  return oa > ba || (oa == ba && oi < bi);
}

// ---- load: working frame = source (+ mirror of the lower triangle) + damping, identity padding --------------------------
template <typename T>
__global__ __launch_bounds__(256) void lu_load_kernel(const T* __restrict__ M, int64_t mrs, int64_t mbs, int sym,
                                                      const T* __restrict__ damping, int ellipsoidal, T eps,
                                                      T* __restrict__ LU, int64_t ld, int n, int nb) {
  __shared__ T s[NB][BLS];
  const int b = blockIdx.x / (nb * nb), t = blockIdx.x % (nb * nb);
  const int bi = t / nb, bj = t % nb, tx = threadIdx.x, ty = threadIdx.y;
  const bool mirror = sym && bi < bj;
  const int si = mirror ? bj : bi, sj = mirror ? bi : bj;
  const T* Mb = M + (int64_t)b * mbs;
  T* Lb = LU + (int64_t)b * ld * ld;
  for (int i = ty; i < NB; i += 8) {
    const int r = NB * si + i, c = NB * sj + tx;
    s[i][tx] = (r < n && c < n) ? Mb[(int64_t)r * mrs + c] : T(0);
  }
  __syncthreads();
  for (int i = ty; i < NB; i += 8) {
    const int r = NB * bi + i, c = NB * bj + tx;
    T v;
    if (r < n && c < n) {
      if (!sym || bi > bj) v = s[i][tx];
      else if (bi < bj) v = s[tx][i];
      else v = i >= tx ? s[i][tx] : s[tx][i];
      if (r == c && damping) {
        const T lam = damping[b];
        v = ellipsoidal ? v + (lam * v + eps) : v + lam;
      }
    } else {
      v = r == c ? T(1) : T(0);
    }
    Lb[(int64_t)r * ld + c] = v;
  }
}

// ---- panel factorisation -----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PANEL_NT) void lu_panel_kernel(T* __restrict__ LU, int64_t ld, int n, int k0,
                                                            int32_t* __restrict__ piv, int32_t* __restrict__ info) {
  __shared__ T s_abs[PANEL_NT / 64], s_val[PANEL_NT / 64];
  __shared__ int s_idx[PANEL_NT / 64];
  __shared__ T s_rowP[SUBW], s_rowK[SUBW];
  __shared__ T s_U[SUBW][NB - SUBW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T* A = LU + (int64_t)b * ld * ld;
  const int kb = min(NB, n - k0);
  int bad = 0;
  if (tid == 0 && k0 != 0) bad = info[b];

#pragma unroll
  for (int s = 0; s < NB / SUBW; ++s) {
    const int c0 = SUBW * s;
    if (c0 < kb) {   // (uniform)
      T a[PANEL_ROWS][SUBW];
#pragma unroll
      for (int q = 0; q < PANEL_ROWS; ++q) {
        const int r = k0 + tid + PANEL_NT * q;
#pragma unroll
        for (int c = 0; c < SUBW; ++c) a[q][c] = r < n ? A[(int64_t)r * ld + k0 + c0 + c] : T(0);
      }
#pragma unroll
      for (int c = 0; c < SUBW; ++c) {
        const int cg = c0 + c;
        if (cg < kb) {   // (uniform)
          const int kr = k0 + cg;
          T bv = T(0), ba = T(-1);
          int bi = 0x7fffffff;
#pragma unroll
          for (int q = 0; q < PANEL_ROWS; ++q) {   // ascending rows, strict >: the lowest row of equal magnitudes stays
            const int r = k0 + tid + PANEL_NT * q;
            const T av = absval(a[q][c]);
            if (r >= kr && r < n && av > ba) {
              ba = av;
              bv = a[q][c];
              bi = r;
            }
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const T oa = __shfl_xor(ba, off), ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (pivot_beats(oa, oi, ba, bi)) {
              ba = oa;
              bv = ov;
              bi = oi;
            }
          }
          if (lane == 0) {
            s_abs[wave] = ba;
            s_val[wave] = bv;
            s_idx[wave] = bi;
          }
          __syncthreads();
          ba = s_abs[0];
          bv = s_val[0];
          bi = s_idx[0];
#pragma unroll
          for (int w = 1; w < PANEL_NT / 64; ++w) {
            const T oa = s_abs[w];
            const int oi = s_idx[w];
            if (pivot_beats(oa, oi, ba, bi)) {
              ba = oa;
              bv = s_val[w];
              bi = oi;
            }
          }
          // (a column of NaNs leaves no candidate: keep the row where it is)
          const int p = bi == 0x7fffffff ? kr : bi;
          const T pv = bv;
          if (tid == 0) {
            piv[(int64_t)b * n + kr] = p;
            if (pv == T(0) && bad == 0) bad = kr + 1;
          }
          // row interchange kr <-> p: the register columns through LDS, the panel's other columns in global memory
          const int lk = kr - k0, lp = p - k0;
#pragma unroll
          for (int q = 0; q < PANEL_ROWS; ++q) {
            const int lr = tid + PANEL_NT * q;
            if (lr == lp) {
#pragma unroll
              for (int cc = 0; cc < SUBW; ++cc) s_rowP[cc] = a[q][cc];
            }
            if (lr == lk) {
#pragma unroll
              for (int cc = 0; cc < SUBW; ++cc) s_rowK[cc] = a[q][cc];
            }
          }
          if (p != kr && tid < NB && (tid < c0 || tid >= c0 + SUBW)) {
            T* x = A + (int64_t)kr * ld + k0 + tid;
            T* y = A + (int64_t)p * ld + k0 + tid;
            const T tmp = *x;
            *x = *y;
            *y = tmp;
          }
          __syncthreads();
#pragma unroll
          for (int q = 0; q < PANEL_ROWS; ++q) {
            const int lr = tid + PANEL_NT * q;
            if (lr == lk) {
#pragma unroll
              for (int cc = 0; cc < SUBW; ++cc) a[q][cc] = s_rowP[cc];
            } else if (lr == lp) {
#pragma unroll
              for (int cc = 0; cc < SUBW; ++cc) a[q][cc] = s_rowK[cc];
            }
          }
          if (pv != T(0)) {   // an exactly zero pivot: nothing below it either, no division
#pragma unroll
            for (int q = 0; q < PANEL_ROWS; ++q) {
              const int r = k0 + tid + PANEL_NT * q;
              if (r > kr && r < n) {
                const T l = a[q][c] / pv;
                a[q][c] = l;
#pragma unroll
                for (int cc = c + 1; cc < SUBW; ++cc) a[q][cc] -= l * s_rowP[cc];
              }
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < PANEL_ROWS; ++q) {
        const int r = k0 + tid + PANEL_NT * q;
        if (r < n) {
#pragma unroll
          for (int c = 0; c < SUBW; ++c) A[(int64_t)r * ld + k0 + c0 + c] = a[q][c];
        }
      }
      __syncthreads();
      constexpr int REM_MAX = NB - SUBW;
      const int rem = NB - c0 - SUBW;   // panel columns right of the register columns
      if (rem > 0) {
        const int t0 = k0 + c0;   // first row / column of the eight just factorised
        if (tid < rem) {          // unit-lower 8 x 8 solve of one column
          T x[SUBW];
#pragma unroll
          for (int j = 0; j < SUBW; ++j) x[j] = A[(int64_t)(t0 + j) * ld + t0 + SUBW + tid];
#pragma unroll
          for (int j = 1; j < SUBW; ++j) {
#pragma unroll
            for (int i = 0; i < j; ++i) x[j] -= A[(int64_t)(t0 + j) * ld + t0 + i] * x[i];
          }
#pragma unroll
          for (int j = 0; j < SUBW; ++j) {
            A[(int64_t)(t0 + j) * ld + t0 + SUBW + tid] = x[j];
            s_U[j][tid] = x[j];
          }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PANEL_ROWS; ++q) {
          const int r = k0 + tid + PANEL_NT * q;
          if (r >= t0 + SUBW && r < n) {
            T* row = A + (int64_t)r * ld + t0 + SUBW;
#pragma unroll
            for (int cc = 0; cc < REM_MAX; ++cc) {
              if (cc < rem) {
                T acc = row[cc];
#pragma unroll
                for (int j = 0; j < SUBW; ++j) acc -= a[q][j] * s_U[j][cc];
                row[cc] = acc;
              }
            }
          }
        }
        __syncthreads();
      }
    }
  }
  if (tid == 0) info[b] = bad;
}

// ---- row interchanges outside the panel + U12 = L11^-1 A12 ---------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void lu_swap_trsm_kernel(T* __restrict__ LU, int64_t ld, int n, int k0, int nblk,
                                                          const int32_t* __restrict__ piv) {
  using M = Mma<T>;
  __shared__ T sL[NB * BLS], sX[NB * BLS], sA[NB * BLS], sU[NB * BLS];
  const int b = blockIdx.x / nblk, jb = blockIdx.x % nblk, lane = threadIdx.x;
  if (jb == k0 / NB) return;
  T* A = LU + (int64_t)b * ld * ld;
  const int kb = min(NB, n - k0), cbase = NB * jb;
  if (lane < NB) {
    const int32_t* pb = piv + (int64_t)b * n + k0;
    for (int c = 0; c < kb; ++c) {
      const int p = pb[c];
      if (p != k0 + c) {
        T* x = A + (int64_t)(k0 + c) * ld + cbase + lane;
        T* y = A + (int64_t)p * ld + cbase + lane;
        const T tmp = *x;
        *x = *y;
        *y = tmp;
      }
    }
  }
  if (jb < k0 / NB) return;
  __syncthreads();
  for (int idx = lane; idx < NB * NB; idx += 64) {
    const int i = idx >> 5, k = idx & 31;
    sL[i * BLS + k] = k < i ? A[(int64_t)(k0 + i) * ld + k0 + k] : (k == i ? T(1) : T(0));
    sA[i * BLS + k] = A[(int64_t)(k0 + i) * ld + cbase + k];
  }
  __syncthreads();
  if (lane < NB) {   // column `lane` of X = L11^-1 (unit lower)
    T x[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      T acc = i == lane ? T(1) : T(0);
#pragma unroll
      for (int k = 0; k < i; ++k) acc -= sL[i * BLS + k] * x[k];
      x[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) sX[i * BLS + lane] = x[i];
  }
  __syncthreads();
  typename M::Frag d;
#pragma unroll
  for (int e = 0; e < 16; ++e) M::set(d, e, T(0));
  M::mac(d, sX, BLS, sA, BLS, T(1), lane);   // U = X A
#pragma unroll
  for (int e = 0; e < 16; ++e) sU[M::row(e, lane) * BLS + M::col(e, lane)] = M::get(d, e);
  __syncthreads();
  // (every product is accumulated from zero and added once: an accumulator that starts from the addend rounds at the addend's
  //  magnitude in each of the 16 MFMA steps)
  typename M::Frag r;
#pragma unroll
  for (int e = 0; e < 16; ++e) M::set(r, e, T(0));
  M::mac(r, sL, BLS, sU, BLS, T(1), lane);   // L11 U
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) {   // R = A - L11 U  (a lane reads and writes its own elements of sA)
    const int o = M::row(e, lane) * BLS + M::col(e, lane);
    sA[o] = sA[o] - M::get(r, e);
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) M::set(r, e, T(0));
  M::mac(r, sX, BLS, sA, BLS, T(1), lane);   // X R
#pragma unroll
  for (int e = 0; e < 16; ++e)               // U += X R
    A[(int64_t)(k0 + M::row(e, lane)) * ld + cbase + M::col(e, lane)] = M::get(d, e) + M::get(r, e);
}

// ---- trailing update A22 -= L21 U12 ---------------------------------------------------------------------------------------
constexpr int TR = 128, TC = 64, TCS = TC + 4;

template <typename T>
__global__ __launch_bounds__(256) void lu_trailing_kernel(T* __restrict__ LU, int64_t ld, int n32, int k0, int tr, int tc) {
  using M = Mma<T>;
  __shared__ T sL[TR * BLS], sU[NB * TCS];
  const int per = tr * tc, b = blockIdx.x / per, t = blockIdx.x % per;
  const int r0 = k0 + NB + TR * (t / tc), c0 = k0 + NB + TC * (t % tc);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T* A = LU + (int64_t)b * ld * ld;
  for (int idx = tid; idx < TR * NB; idx += 256) {
    const int i = idx >> 5, k = idx & 31;
    sL[i * BLS + k] = r0 + i < n32 ? A[(int64_t)(r0 + i) * ld + k0 + k] : T(0);
  }
  for (int idx = tid; idx < NB * TC; idx += 256) {
    const int k = idx / TC, j = idx % TC;
    sU[k * TCS + j] = c0 + j < n32 ? A[(int64_t)(k0 + k) * ld + c0 + j] : T(0);
  }
  __syncthreads();
  const int rw = r0 + NB * wave;
  if (rw >= n32) return;
#pragma unroll
  for (int jb = 0; jb < TC / NB; ++jb) {
    const int cw = c0 + NB * jb;
    if (cw < n32) {   // (wave uniform)
      typename M::Frag d;   // the product from zero, subtracted once (see lu_swap_trsm_kernel); A22 is in flight meanwhile
      T c[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        c[e] = A[(int64_t)(rw + M::row(e, lane)) * ld + cw + M::col(e, lane)];
        M::set(d, e, T(0));
      }
      M::mac(d, sL + NB * wave * BLS, BLS, sU + NB * jb, TCS, T(1), lane);
#pragma unroll
      for (int e = 0; e < 16; ++e) A[(int64_t)(rw + M::row(e, lane)) * ld + cw + M::col(e, lane)] = c[e] - M::get(d, e);
    }
  }
}

// ---- solves: one workgroup per problem, the vector in LDS ------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

template <typename T>
__device__ __forceinline__ void stage_diag_block(const T* A, int64_t ld, int r0, T* sD, int tid) {
  for (int idx = tid; idx < NB * NB; idx += 256) {
    const int i = idx >> 5, k = idx & 31;
    sD[i * BLS + k] = A[(int64_t)(r0 + i) * ld + r0 + k];
  }
}

// y = L^-1 P rhs
template <typename T>
__global__ __launch_bounds__(256) void lu_fwd_kernel(const T* __restrict__ LU, int64_t ld, int n, int n32,
                                                     const int32_t* __restrict__ piv, const T* rhs, T* y, int64_t ldv) {
  extern __shared__ __align__(16) unsigned char lu_smem[];
  T* v = reinterpret_cast<T*>(lu_smem);
  T* sD = v + n32;
  T* sdot = sD + NB * BLS;
  int* sp = reinterpret_cast<int*>(sdot + NB);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* A = LU + (int64_t)b * ld * ld;
  for (int i = tid; i < n32; i += 256) v[i] = i < n ? rhs[(int64_t)b * ldv + i] : T(0);
  for (int i = tid; i < n; i += 256) sp[i] = piv[(int64_t)b * n + i];
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < n; ++k) {
      const int p = sp[k];
      if (p != k && (unsigned)p < (unsigned)n) {
        const T tmp = v[k];
        v[k] = v[p];
        v[p] = tmp;
      }
    }
  }
  __syncthreads();
  for (int r0 = 0; r0 < n32; r0 += NB) {
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 8 * wave + i;
      T s = T(0);
      for (int k = lane; k < r0; k += 64) s += A[(int64_t)r * ld + k] * v[k];
      s = wave_sum(s);
      if (lane == 0) sdot[8 * wave + i] = s;
    }
    stage_diag_block(A, ld, r0, sD, tid);
    __syncthreads();
    if (wave == 0) {
      const int i = lane & 31;
      T yi = v[r0 + i] - sdot[i];
#pragma unroll
      for (int k = 0; k < NB - 1; ++k) {
        const T yk = __shfl(yi, k);
        if (i > k) yi -= sD[i * BLS + k] * yk;
      }
      if (lane < NB) v[r0 + i] = yi;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += 256) y[(int64_t)b * ldv + i] = v[i];
}

// x = U^-1 y
template <typename T>
__global__ __launch_bounds__(256) void lu_bwd_kernel(const T* __restrict__ LU, int64_t ld, int n, int n32, const T* y, T* x,
                                                     int64_t ldv) {
  extern __shared__ __align__(16) unsigned char lu_smem[];
  T* v = reinterpret_cast<T*>(lu_smem);
  T* sD = v + n32;
  T* sdot = sD + NB * BLS;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* A = LU + (int64_t)b * ld * ld;
  for (int i = tid; i < n32; i += 256) v[i] = i < n ? y[(int64_t)b * ldv + i] : T(0);
  __syncthreads();
  for (int r0 = n32 - NB; r0 >= 0; r0 -= NB) {
    for (int i = 0; i < 8; ++i) {
      const int r = r0 + 8 * wave + i;
      T s = T(0);
      for (int k = r0 + NB + lane; k < n32; k += 64) s += A[(int64_t)r * ld + k] * v[k];
      s = wave_sum(s);
      if (lane == 0) sdot[8 * wave + i] = s;
    }
    stage_diag_block(A, ld, r0, sD, tid);
    __syncthreads();
    if (wave == 0) {
      const int i = lane & 31;
      T xi = v[r0 + i] - sdot[i];
#pragma unroll
      for (int k = NB - 1; k >= 0; --k) {
        if (i == k) xi = xi / sD[k * BLS + k];
        const T xk = __shfl(xi, k);
        if (i < k) xi -= sD[i * BLS + k] * xk;
      }
      if (lane < NB) v[r0 + i] = xi;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += 256) x[(int64_t)b * ldv + i] = v[i];
}

static inline size_t lu_solve_lds(int n, int n32, size_t elem) { return (size_t)(n32 + NB * BLS + NB) * elem + (size_t)n * sizeof(int); }

template <typename T>
int lu_factor_impl(const void* M, int64_t ld, int n, int B, int sym, const void* damping, int ellipsoidal, double eps, void* LU,
                   int32_t* piv, int32_t* info, hipStream_t st) {
  const int n32 = (n + NB - 1) / NB * NB, nb = (int)(ld / NB), nblk = n32 / NB;
  if ((int64_t)B * nb * nb > 0x7fffffffLL) return fail("thx_lu_factor: B * (ld / 32)^2 exceeds the grid limit");
  T* lu = static_cast<T*>(LU);
  const int64_t mrs = sym ? ld : n, mbs = mrs * mrs;
  lu_load_kernel<T><<<dim3((unsigned)(B * nb * nb)), dim3(NB, 8), 0, st>>>(static_cast<const T*>(M), mrs, mbs, sym,
                                                                            static_cast<const T*>(damping), ellipsoidal, (T)eps,
                                                                            lu, ld, n, nb);
  for (int k0 = 0; k0 < n; k0 += NB) {
    lu_panel_kernel<T><<<dim3(B), dim3(PANEL_NT), 0, st>>>(lu, ld, n, k0, piv, info);
    if (nblk > 1) lu_swap_trsm_kernel<T><<<dim3((unsigned)(B * nblk)), dim3(64), 0, st>>>(lu, ld, n, k0, nblk, piv);
    const int m = n32 - k0 - NB;
    if (m > 0) {
      const int tr = (m + TR - 1) / TR, tc = (m + TC - 1) / TC;
      lu_trailing_kernel<T><<<dim3((unsigned)(B * tr * tc)), dim3(256), 0, st>>>(lu, ld, n32, k0, tr, tc);
    }
  }
  return check_launch("thx_lu_factor");
}

template <typename T>
int lu_solve_impl(const void* LU, int64_t ld, int n, int B, const int32_t* piv, const void* rhs, void* x, int64_t ldv, bool fwd,
                  bool bwd, hipStream_t st) {
  const int n32 = (n + NB - 1) / NB * NB;
  const size_t lds = lu_solve_lds(n, n32, sizeof(T));
  const T* lu = static_cast<const T*>(LU);
  const T* in = static_cast<const T*>(rhs);
  if (fwd) {
    lu_fwd_kernel<T><<<dim3(B), dim3(256), lds, st>>>(lu, ld, n, n32, piv, in, static_cast<T*>(x), ldv);
    in = static_cast<const T*>(x);
  }
  if (bwd) lu_bwd_kernel<T><<<dim3(B), dim3(256), lds, st>>>(lu, ld, n, n32, in, static_cast<T*>(x), ldv);
  return check_launch("thx_lu_solve");
}

static int check_lu_sizes(const char* who, int n, int B, int64_t ld) {
  if (n <= 0 || B <= 0 || ld < n || (ld % 32) != 0) return fail(who, ": need n>0, B>0, ld>=n, ld%32==0");
  if (n > LU_MAX_N || ld > LU_MAX_N) return fail(who, ": n (and ld) above the limit of 4096 of the dense LU");
  return 0;
}

static int lu_solve_dispatch(const char* who, const void* LU, int64_t ld, int n, int B, const int32_t* piv, const void* rhs, void* x,
                      int64_t ldv, bool fwd, bool bwd, int dtype, void* stream) {
  if (!LU || !rhs || !x || (fwd && !piv)) return fail(who, ": null pointer");
  if (int r = check_lu_sizes(who, n, B, ld)) return r;
  if (ldv < n) return fail(who, ": ldv < n");
  THX_DISPATCH(dtype, return lu_solve_impl<float>(LU, ld, n, B, piv, rhs, x, ldv, fwd, bwd, as_stream(stream)),
               return lu_solve_impl<double>(LU, ld, n, B, piv, rhs, x, ldv, fwd, bwd, as_stream(stream)));
  return 0;
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_lu_factor(const void* M, int64_t ld, int32_t n, int32_t B, int symmetric_lower, const void* damping, int ellipsoidal,
                  double damping_eps, void* LU, int32_t* piv, int32_t* info, int dtype, void* stream) {
  if (!M || !LU || !piv || !info) return fail("thx_lu_factor: null pointer");
  if (int r = check_lu_sizes("thx_lu_factor", n, B, ld)) return r;
  if (M == LU) return fail("thx_lu_factor: LU must not alias M (the source stays undamped)");
  THX_DISPATCH(dtype,
               return lu_factor_impl<float>(M, ld, n, B, symmetric_lower != 0, damping, ellipsoidal, damping_eps, LU, piv, info,
                                            as_stream(stream)),
               return lu_factor_impl<double>(M, ld, n, B, symmetric_lower != 0, damping, ellipsoidal, damping_eps, LU, piv, info,
                                             as_stream(stream)));
  return 0;
}

int thx_lu_solve_forward(const void* LU, int64_t ld, int32_t n, int32_t B, const int32_t* piv, const void* rhs, void* y,
                         int64_t ldv, int dtype, void* stream) {
  return lu_solve_dispatch("thx_lu_solve_forward", LU, ld, n, B, piv, rhs, y, ldv, true, false, dtype, stream);
}

int thx_lu_solve_backward(const void* LU, int64_t ld, int32_t n, int32_t B, const void* y, void* x, int64_t ldv, int dtype,
                          void* stream) {
  return lu_solve_dispatch("thx_lu_solve_backward", LU, ld, n, B, nullptr, y, x, ldv, false, true, dtype, stream);
}

int thx_lu_solve(const void* LU, int64_t ld, int32_t n, int32_t B, const int32_t* piv, const void* rhs, void* x, int64_t ldv,
                 int dtype, void* stream) {
  return lu_solve_dispatch("thx_lu_solve", LU, ld, n, B, piv, rhs, x, ldv, true, true, dtype, stream);
}

}  // extern "C"
