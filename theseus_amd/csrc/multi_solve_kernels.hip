// Triangular solves with a BLOCK of right-hand sides against a dense-frame Cholesky factor, for gfx950:
//   X = (L L^T)^-1 R,  X = L^-T R  or  X = L^-1 R   for R = (B, nrhs, n), one vector per row.
// What TheseusLayer.compute_samples (theseus/theseus_layer.py:99-135: delta + L^-T y for a block of normal draws y) and
// marginal covariances (blocks of H^-1: a solve against unit vectors) need from the factor the optimiser already holds.  The
// single-vector solves of chol_kernels.hip stream every tile of L once per vector; here a workgroup streams L once per GROUP
// of up to 32 vectors and the products run on the matrix cores.
//
// One 256-thread workgroup per (problem, group of 32 right-hand sides); groups never interact.  The block of vectors stays in x
// (global memory / L2), as thx_chol_solve_sparse keeps its vector; on chip are only the accumulator of the current block row
// (128 x 32, a 32 x 32 fragment per wave), one 128 x 32 chunk of L and one 32 x 32 chunk of X in LDS.
//   forward, block row i:  T = R_i - sum_{j<i} L_ij X_j        chunks of 32 columns of L_ij (A operand) x 32 rows of X_j (B operand)
//                          through the Winv panel of the diagonal tile, 32 rows at a time:  x_s = W_ss t_s ;  t_u += (-L_us) x_s, u > s
//   backward, block row i: T = Z_i - sum_{j>i} L_ji^T X_j      chunks of 32 ROWS of L_ji, read as they lie and used transposed
//                          x_s = W_ss^T t_s ;  t_u += (-L_su)^T x_s, u < s,  s = 3..0
// The panel's block column (forward) / block row (backward) s is staged with the same code as a chunk of L.  The next chunk is
// in flight in registers while the matrix cores work on the current one.
// Rows / columns >= n of L and of the panel are masked when they are loaded (never multiplied): the padding of the frame may hold
// anything.  A partial group's missing vectors are zero columns of the B operand and are never stored; MFMA output columns do
// not mix, so a vector's result does not depend on what else is in the call.
#include <cstdint>

#include "common.cuh"

namespace thx {

constexpr int MS_TILE = 128;             // block row (THX_TILE)
constexpr int MS_KC = 32;                // K extent of a chunk
constexpr int MS_G = 32;                 // right-hand sides per workgroup
constexpr int MS_LSA = MS_KC + 1;        // chunk of L as it is multiplied forward: sA[r * MS_LSA + k], r < 128, k < 32
constexpr int MS_LST = MS_TILE + 4;      // chunk of L read as rows, used transposed: sA[k * MS_LST + r]
constexpr int MS_LSB = MS_G + 1;         // chunk of X: sB[k * MS_LSB + s]
constexpr int MS_SA = MS_TILE * MS_LSA;  // (= 4224 = MS_KC * MS_LST)
static_assert(MS_SA == MS_KC * MS_LST, "one buffer serves both layouts");

typedef float ms_f32x16 __attribute__((ext_vector_type(16)));
typedef double ms_f64x4 __attribute__((ext_vector_type(4)));

// One wave's 32 x 32 (x 32) product on the matrix cores, D += A B.  A(i, k) = sA[i * AIS + k * AKS], B(k, j) = sB[k * MS_LSB + j].
// A lane holds 16 elements of D; element e sits at (row(e, lane), col(e, lane)).
template <typename T>
struct MsMma;

template <>
struct MsMma<float> {   // v_mfma_f32_32x32x2_f32: lane (i = l & 31, k = l >> 5) of A, (k, j = l & 31) of B
  using Frag = ms_f32x16;
  static __device__ __forceinline__ int row(int e, int l) { return 8 * (e >> 2) + 4 * (l >> 5) + (e & 3); }
  static __device__ __forceinline__ int col(int, int l) { return l & 31; }
  static __device__ __forceinline__ float get(const Frag& d, int e) { return d[e]; }
  static __device__ __forceinline__ void set(Frag& d, int e, float x) { d[e] = x; }
  template <int AIS, int AKS>
  static __device__ __forceinline__ void mac(Frag& d, const float* sA, const float* sB, int l) {
    const int i = l & 31, g = l >> 5;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 2 * kk + g;
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[i * AIS + k * AKS], sB[k * MS_LSB + i], d, 0, 0, 0);
    }
  }
};

template <>
struct MsMma<double> {   // v_mfma_f64_16x16x4_f64, two 16-column halves of two 16-row halves: lane (i = l & 15, k = l >> 4)
  struct Frag {
    ms_f64x4 v[4];   // block (ih, jh) = v[2 ih + jh]
  };
  static __device__ __forceinline__ int row(int e, int l) { return 16 * (e >> 3) + 4 * (e & 3) + (l >> 4); }
  static __device__ __forceinline__ int col(int e, int l) { return 16 * ((e >> 2) & 1) + (l & 15); }
  static __device__ __forceinline__ double get(const Frag& d, int e) { return d.v[e >> 2][e & 3]; }
  static __device__ __forceinline__ void set(Frag& d, int e, double x) { d.v[e >> 2][e & 3] = x; }
  template <int AIS, int AKS>
  static __device__ __forceinline__ void mac(Frag& d, const double* sA, const double* sB, int l) {
    const int i = l & 15, g = l >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + g;
      const double a0 = sA[i * AIS + k * AKS], a1 = sA[(16 + i) * AIS + k * AKS];
      const double b0 = sB[k * MS_LSB + i], b1 = sB[k * MS_LSB + 16 + i];
      d.v[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, d.v[0], 0, 0, 0);
      d.v[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, d.v[1], 0, 0, 0);
      d.v[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, d.v[2], 0, 0, 0);
      d.v[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d.v[3], 0, 0, 0);
    }
  }
};

template <typename T>
struct MsVec;
template <>
struct MsVec<float> {
  using V = float4;
  static constexpr int NV = 4;
  static __device__ __forceinline__ float at(const V& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
  static __device__ __forceinline__ V zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <>
struct MsVec<double> {
  using V = double2;
  static constexpr int NV = 2;
  static __device__ __forceinline__ double at(const V& v, int e) { return e == 0 ? v.x : v.y; }
  static __device__ __forceinline__ V zero() { return make_double2(0.0, 0.0); }
};

// One substitution over all block rows of one (problem, group): BWD = false: out = L^-1 in, BWD = true: out = L^-T in.
// `in` is read one block row at a time, just before that block row of `out` is written: out may be in.
template <typename T, bool BWD>
__device__ __forceinline__ void ms_pass(const T* __restrict__ Lb, int64_t ld, int n, int nt, const T* __restrict__ Pb, const T* in,
                                        T* out, int nc, int64_t ldv, T* sA, T* sB, int tid) {
  using M = MsMma<T>;
  using VT = MsVec<T>;
  using V = typename VT::V;
  constexpr int NV = VT::NV;
  constexpr int NL = MS_TILE * MS_KC / NV / 256;       // 16-byte loads of a thread per chunk of L (4 / 8)
  constexpr int AIS = BWD ? 1 : MS_LSA, AKS = BWD ? MS_LST : 1;
  constexpr int VPR = (BWD ? MS_TILE : MS_KC) / NV;    // 16-byte vectors per row of a chunk as it lies in memory
  const int wave = tid >> 6, lane = tid & 63;
  const int bs = tid >> 3, bk = (tid & 7) * 4;         // this thread's vector and first row of a chunk of X

  for (int q = 0; q < nt; ++q) {
    const int ib = BWD ? nt - 1 - q : q, row0 = ib * MS_TILE, valid = min(MS_TILE, n - row0);
    // chunks of the block row: nch of the off-diagonal tiles (K ascending), then the four of the diagonal tile's panel
    const int nch = BWD ? (max(n - (row0 + MS_TILE), 0) + MS_KC - 1) / MS_KC : row0 / MS_KC;
    const T* Pn = Pb + (int64_t)ib * MS_TILE * MS_TILE;
    V ra[NL];
    T rb[4];
    // chunk c -> registers.  Off-diagonal: K rows / columns k0..k0+31 of L and of X.  Panel: block column (row) s of it.
    auto load = [&](int c) __attribute__((always_inline)) {
      const bool diag = c >= nch;
      const int s = BWD ? 3 - (c - nch) : c - nch;
      const int k0 = BWD ? row0 + MS_TILE + MS_KC * c : MS_KC * c;
#pragma unroll
      for (int u = 0; u < NL; ++u) {
        const int v = tid + 256 * u, a = v / VPR, bq = (v % VPR) * NV;   // element (a, bq..) of the chunk as it lies in memory
        const int r = BWD ? bq : a, k = BWD ? a : bq;                     // (r: row of the block row, k: K index; NV along one)
        V val = VT::zero();
        if (!diag) {
          // forward L[row0 + r][k0 + k..]: rows < n;  backward L[k0 + k][row0 + r..]: rows < n (columns are below row0 + 128 <= n)
          if (BWD ? (k0 + k < n) : (r < valid))
            val = *reinterpret_cast<const V*>(BWD ? Lb + (int64_t)(k0 + k) * ld + row0 + r : Lb + (int64_t)(row0 + r) * ld + k0 + k);
        } else {
          const V pv = *reinterpret_cast<const V*>(BWD ? Pn + (MS_KC * s + k) * MS_TILE + r : Pn + r * MS_TILE + MS_KC * s + k);
          // the panel is 128 x 128 whatever n is; only rows and columns < valid belong to the matrix
          const bool rowok = (BWD ? MS_KC * s + k : r) < valid;
          T e[NV];
#pragma unroll
          for (int i = 0; i < NV; ++i) e[i] = (rowok && (BWD ? r + i : MS_KC * s + k + i) < valid) ? VT::at(pv, i) : T(0);
          if constexpr (NV == 4) val = V{e[0], e[1], e[2], e[3]};
          else val = V{e[0], e[1]};
        }
        ra[u] = val;
      }
      if (!diag) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rb[i] = (bs < nc && k0 + bk + i < n) ? out[(int64_t)bs * ldv + k0 + bk + i] : T(0);
      }
    };
    auto store = [&](int c) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < NL; ++u) {
        const int v = tid + 256 * u, a = v / VPR, bq = (v % VPR) * NV;
#pragma unroll
        for (int i = 0; i < NV; ++i) sA[a * (BWD ? MS_LST : MS_LSA) + bq + i] = VT::at(ra[u], i);
      }
      if (c < nch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sB[(bk + i) * MS_LSB + bs] = rb[i];
      }
    };

    typename M::Frag acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) M::set(acc, e, T(0));
    load(0);
    for (int c = 0; c < nch + 4; ++c) {
      __syncthreads();   // the previous chunk has been consumed; block rows of `out` written so far are visible to the workgroup
      const bool diag = c >= nch;
      const int s = BWD ? 3 - (c - nch) : c - nch;
      if (c == nch) {    // T = in_i - (product accumulated from zero)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = MS_KC * wave + M::row(e, lane), j = M::col(e, lane);
          const T v = (r < valid && j < nc) ? in[(int64_t)j * ldv + row0 + r] : T(0);
          M::set(acc, e, v - M::get(acc, e));
        }
      }
      store(c);
      if (diag && wave == s) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sB[M::row(e, lane) * MS_LSB + M::col(e, lane)] = M::get(acc, e);
      }
      __syncthreads();
      if (c + 1 < nch + 4) load(c + 1);
      const T* sAw = sA + MS_KC * wave * AIS;   // this wave's 32 rows of the block row
      if (!diag) {
        M::template mac<AIS, AKS>(acc, sAw, sB, lane);
      } else {
        // x_s = W_ss t_s  (backward: W_ss^T t_s) by wave s, then t_u += (-L_us) x_s (backward: (-L_su)^T x_s) by the waves still open
        if (wave == s) {
          typename M::Frag xs;
#pragma unroll
          for (int e = 0; e < 16; ++e) M::set(xs, e, T(0));
          M::template mac<AIS, AKS>(xs, sAw, sB, lane);
          acc = xs;
        }
        __syncthreads();   // t_s has been read by all lanes of wave s
        if (wave == s) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = M::row(e, lane), j = M::col(e, lane), r = MS_KC * s + rl;
            const T v = M::get(acc, e);
            sB[rl * MS_LSB + j] = v;
            if (r < valid && j < nc) out[(int64_t)j * ldv + row0 + r] = v;
          }
        }
        __syncthreads();
        if (BWD ? wave < s : wave > s) M::template mac<AIS, AKS>(acc, sAw, sB, lane);
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
chol_solve_multi_kernel(const T* __restrict__ L, int64_t ld, int n, const T* __restrict__ Winv, const T* rhs, T* x, int nrhs,
                        int64_t ldv, int64_t bstride, int ngroups, int fwd, int bwd) {
  __shared__ __attribute__((aligned(16))) T sA[MS_SA];
  __shared__ T sB[MS_KC * MS_LSB];
  const int b = blockIdx.x / ngroups, g = blockIdx.x % ngroups, tid = threadIdx.x;
  const int nt = (n + MS_TILE - 1) / MS_TILE, nc = min(MS_G, nrhs - MS_G * g);
  const T* Lb = L + (int64_t)b * ld * ld;
  const T* Pb = Winv + (int64_t)b * nt * MS_TILE * MS_TILE;
  const T* in = rhs + (int64_t)b * bstride + (int64_t)MS_G * g * ldv;
  T* out = x + (int64_t)b * bstride + (int64_t)MS_G * g * ldv;
  if (fwd) {
    ms_pass<T, false>(Lb, ld, n, nt, Pb, in, out, nc, ldv, sA, sB, tid);
    in = out;
  }
  if (bwd) ms_pass<T, true>(Lb, ld, n, nt, Pb, in, out, nc, ldv, sA, sB, tid);
}

template <typename T>
static int solve_multi_impl(const void* L, int64_t ld, int n, int B, const void* Winv, const void* rhs, void* x, int nrhs, int64_t ldv,
                            int64_t bstride, int which, hipStream_t st) {
  const int ngroups = (int)(((int64_t)nrhs + MS_G - 1) / MS_G);
  chol_solve_multi_kernel<T><<<dim3((unsigned)(B * ngroups)), dim3(256), 0, st>>>(
      static_cast<const T*>(L), ld, n, static_cast<const T*>(Winv), static_cast<const T*>(rhs), static_cast<T*>(x), nrhs, ldv,
      bstride, ngroups, which != 1, which != 2);
  return check_launch("thx_chol_solve_multi");
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_chol_solve_multi(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x, int32_t nrhs,
                         int64_t ldv, int64_t bstride, int which, int dtype, void* stream) {
  const char* who = "thx_chol_solve_multi";
  if (!L || !Winv || !rhs || !x) return fail(who, ": null pointer");
  if (n <= 0 || B <= 0 || ld < n || (ld % 32) != 0) return fail(who, ": need n>0, B>0, ld>=n, ld%32==0 (a dense factor frame)");
  if (nrhs < 1) return fail(who, ": nrhs < 1");
  if (ldv < n) return fail(who, ": ldv < n");
  if (bstride / nrhs < ldv) return fail(who, ": bstride < nrhs * ldv");   // (no product: nrhs * ldv may not fit)
  if (which < 0 || which > 2) return fail(who, ": which = 0 (both), 1 (backward only), 2 (forward only)");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if ((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Winv)) % 16) return fail(who, ": L and Winv must be 16-byte aligned");
  if ((int64_t)B * (((int64_t)nrhs + MS_G - 1) / MS_G) > 0x7fffffffLL) return fail(who, ": B * ceil(nrhs / 32) exceeds the grid limit");
  THX_DISPATCH(dtype, return solve_multi_impl<float>(L, ld, n, B, Winv, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)),
               return solve_multi_impl<double>(L, ld, n, B, Winv, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)));
  return 0;
}

}  // extern "C"
