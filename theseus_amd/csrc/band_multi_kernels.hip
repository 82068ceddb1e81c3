// Blocks of right-hand sides and the band of the inverse on the banded Cholesky factor Lb of thx_band_factor (band_kernels.hip),
// gfx950: what posterior samples (delta + L^-T y) and marginal covariances (blocks of (L L^T)^-1) need from that factor.
//
// pb_solve_multi_kernel  ONE WAVE PER (problem, group of up to 64 vectors), LANE = VECTOR.  The single-vector kernels pay a division,
//                        a v_readlane and an fma on the chain from column j to j + 1, because the lanes share one vector; here a lane
//                        owns a whole vector, every value it needs is its own, and the step from one column to the next has no
//                        cross-lane instruction and no reduction.
//                        Forward (y = L^-1 P rhs), column oriented: a ring of kd + 1 pending SUMS per lane (slot r mod (kd + 1) is
//                        row r's), y_j = (b_j - sum_j) / d_j, then sum_(j+i) += Lb[j, i] y_j for the contiguous column j: kd
//                        independent fmas.  Backward (x = L^-T y): x_j = (y_j - sum_i Lb[j, i] x_(j+i)) / d_j, the dot of column j
//                        with the ring of the last kd results, on four partial sums.  The ring is in REGISTERS for kd <= 7 (eight
//                        slots, the slot of a column is a compile-time index because chunks of eight columns are unrolled) and in
//                        LDS otherwise ([kd + 1][64], lane-consecutive: conflict free, touched by its own lane only: no fences).
//                        Lb is wave-uniform: a chunk of eight columns (8 (kd + 1) contiguous elements) is loaded coalesced into
//                        registers one chunk AHEAD and parked in LDS, the columns are read back as broadcasts.
//                        rhs / x move in tiles of 16 positions x 64 vectors: lanes run along n (through perm where the order asks
//                        for it) and write the tile transposed into LDS (row stride 68: both directions conflict free), the
//                        lane = vector phase reads and overwrites tile[j][lane], the finished tile leaves the same way.  The next
//                        tile is in flight in registers while this one is processed.  A (problem, vector) row belongs to one wave
//                        and a tile's positions are read before they are written, so x may be rhs when both use one order
//                        (which = 0); when the orders differ (which = 1, 2) the aliased call solves in the input's order and then
//                        permutes each row through LDS (n elements).
// pb_inverse_band_kernel ONE WAVE PER PROBLEM (up to four per workgroup, never synchronised): selected inversion (Takahashi's
//                        equations) for the band of S = (L L^T)^-1, columns j = n - 1 .. 0:
//                          S(j + i, j) = -(1 / d) sum_k l_k S(j + k, j + i),   S(j, j) = 1 / d^2 - (1 / d) sum_k l_k S(j + k, j).
//                        The live symmetric window S(j + 1 .. j + kd, j + 1 .. j + kd) sits in LDS on a (kd + 1) x (kd + 1) torus,
//                        element (r, c) at [c mod w][r mod w] with row stride S = w | 1, BOTH triangles: lane i reads
//                        S(j + i, j + k) for k = 1 .. kd, consecutive over the lanes for every k (the symmetric direction: the other
//                        one strides by S - 1, 64 banks apart at kd = 63).  Each dot is one sum, scaled once.  The diagonal is one
//                        wave reduction.  Column j then overwrites column j + kd + 1 (contiguous) and row j + kd + 1 (stride S, odd:
//                        conflict free) and leaves to Zb as one segment.  Columns of Lb are fetched a chunk of eight ahead.
// Every issued load has a clamped address (no load waits behind a branch); no atomics; every output element is written, nothing is
// accumulated in memory.
#include <type_traits>

#include "band_common.cuh"

namespace thx {

constexpr int PBM_TJ = 16;   // positions per transposed tile (two chunks of BAND_CH columns)
constexpr int PBM_TS = 68;   // tile row stride: lane (pos, vq) writes pos * 68 + vec -- 4 pos + vq mod 64, all different
constexpr int PBM_RK = 8;    // register ring slots: kd + 1 <= 8
static_assert(PBM_TJ == 2 * BAND_CH && PBM_RK == BAND_CH, "a column's ring slot is its index in the unrolled chunk");

// per-wave LDS elements of the multi-solve: the tile, one chunk of Lb, the ring (LDS variant)
__host__ __device__ inline size_t pbm_elems(int w, bool lds_ring) {
  return (size_t)PBM_TJ * PBM_TS + (size_t)BAND_CH * w + (lds_ring ? (size_t)w * 64 : 0);
}

template <typename T, bool REG>
__global__ __launch_bounds__(64) void pb_solve_multi_kernel(const T* __restrict__ Lb, int n, int kd, int ngroups,
                                                            const int32_t* __restrict__ perm, const T* rhs, T* x, int nrhs,
                                                            int64_t ldv, int64_t bstride, int which, int alias) {
  extern __shared__ __attribute__((aligned(16))) char pbm_smem[];
  const int lane = threadIdx.x;
  const int b = blockIdx.x / ngroups, g = blockIdx.x - b * ngroups;
  const int w = kd + 1;
  T* tile = reinterpret_cast<T*>(pbm_smem);      // [TJ][TS]
  T* lst = tile + PBM_TJ * PBM_TS;               // [CH][w]: the chunk of Lb being applied
  T* ring = lst + BAND_CH * w;                   // [w][64] (LDS variant)
  const T* Lo = Lb + (int64_t)b * n * w;
  const int64_t lmax = (int64_t)n * w - 1;
  const int v0 = g * 64;
  const int pos = lane & (PBM_TJ - 1), vq = lane >> 4;   // the transposed phase: 16 positions x 4 vectors per pass
  const int ntiles = (n + PBM_TJ - 1) / PBM_TJ;
  const int nl = (BAND_CH * w + 63) >> 6;                // loads per lane and chunk of Lb

  auto load_L = [&](int j0, T(&pre)[BAND_CH]) {          // columns j0 .. j0 + CH - 1, clamped into Lb
#pragma unroll
    for (int q = 0; q < BAND_CH; ++q)
      if (q < nl) {
        int64_t e = (int64_t)j0 * w + q * 64 + lane;
        e = e < 0 ? 0 : (e > lmax ? lmax : e);
        pre[q] = Lo[e];
      }
  };
  auto park_L = [&](const T(&pre)[BAND_CH]) {
#pragma unroll
    for (int q = 0; q < BAND_CH; ++q)
      if (q < nl && q * 64 + lane < BAND_CH * w) lst[q * 64 + lane] = pre[q];
  };
  // element offset of (vector v0 + vec, banded position j) in a (B, nrhs, n) block; through perm when that side is in the
  // linearization's order.  Clamped: a lane outside the block loads what its neighbour loads and never stores.
  auto offset = [&](int vec, int idx) { return (int64_t)b * bstride + (int64_t)min(v0 + vec, nrhs - 1) * ldv + idx; };
  auto load_tile = [&](const T* src, bool through_perm, int j0t, T(&pre)[PBM_TJ]) {
    const int j = min(max(j0t, 0) + pos, n - 1);
    const int idx = through_perm ? perm[j] : j;
#pragma unroll
    for (int it = 0; it < PBM_TJ; ++it) pre[it] = src[offset(it * 4 + vq, idx)];
  };
  auto park_tile = [&](const T(&pre)[PBM_TJ]) {
#pragma unroll
    for (int it = 0; it < PBM_TJ; ++it) tile[pos * PBM_TS + it * 4 + vq] = pre[it];
  };
  auto store_tile = [&](T* dst, bool through_perm, int j0t) {
    const int j = j0t + pos, jc = min(j, n - 1);
    const int idx = through_perm ? perm[jc] : jc;
#pragma unroll
    for (int it = 0; it < PBM_TJ; ++it) {
      const int vec = it * 4 + vq;
      const T v = tile[pos * PBM_TS + vec];
      if (j < n && v0 + vec < nrhs) dst[offset(vec, idx)] = v;
    }
  };

  // one substitution over all columns: FWD ascending, else descending.  Tiles and chunks are aligned at multiples of 16 and 8 in
  // both directions, so column j of an unrolled chunk has the static index cc = j & 7.
  auto sweep = [&](auto fwd_tag, const T* src, bool src_perm, T* dst, bool dst_perm) {
    constexpr bool FWD = decltype(fwd_tag)::value;
    T acc[PBM_RK];                                      // REG: pending sums (forward) / last results (backward), slot = row & 7
#pragma unroll
    for (int k = 0; k < PBM_RK; ++k) acc[k] = T(0);
    if constexpr (!REG)
      for (int k = 0; k < w; ++k) ring[k * 64 + lane] = T(0);
    int jm = FWD ? 0 : (n - 1) % w;                     // LDS ring: slot of column j, j mod w
    T lpre[BAND_CH], tpre[PBM_TJ];
    const int first_tile = FWD ? 0 : (ntiles - 1) * PBM_TJ;
    load_L(FWD ? 0 : first_tile + BAND_CH, lpre);
    load_tile(src, src_perm, first_tile, tpre);
    band_lds_fence();                                   // (whatever the wave read from this LDS before)
    park_L(lpre);
    park_tile(tpre);
    band_lds_fence();
    for (int tt = 0; tt < ntiles; ++tt) {
      const int j0t = FWD ? tt * PBM_TJ : (ntiles - 1 - tt) * PBM_TJ;
      load_tile(src, src_perm, FWD ? j0t + PBM_TJ : j0t - PBM_TJ, tpre);   // (the next tile, in flight under this one)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j0 = j0t + (FWD ? h : 1 - h) * BAND_CH;
        load_L(FWD ? j0 + BAND_CH : j0 - BAND_CH, lpre);                   // (the next chunk of Lb)
#pragma unroll
        for (int c = 0; c < BAND_CH; ++c) {
          const int cc = FWD ? c : BAND_CH - 1 - c, j = j0 + cc;
          if (j < n) {
            const T* lc = lst + cc * w;                 // column j of Lb: broadcasts
            T* mine = tile + (j - j0t) * PBM_TS + lane;
            const T bj = *mine;
            if constexpr (FWD) {
              T yj;
              if constexpr (REG) {
                yj = (bj - acc[cc]) / lc[0];
                acc[cc] = T(0);                         // (row j + 8's from now on)
#pragma unroll
                for (int i = 1; i < PBM_RK; ++i)
                  if (i <= kd) acc[(cc + i) & (PBM_RK - 1)] = fma(lc[i], yj, acc[(cc + i) & (PBM_RK - 1)]);
              } else {
                T* rs = ring + jm * 64 + lane;
                yj = (bj - *rs) / lc[0];
                *rs = T(0);
                int slot = jm;
                for (int i = 1; i <= kd; ++i) {
                  slot = slot + 1 == w ? 0 : slot + 1;
                  T* e = ring + slot * 64 + lane;
                  *e = fma(lc[i], yj, *e);
                }
                jm = jm + 1 == w ? 0 : jm + 1;
              }
              *mine = yj;
            } else {
              T xj;
              if constexpr (REG) {
                T p[2] = {T(0), T(0)};
#pragma unroll
                for (int i = 1; i < PBM_RK; ++i)
                  if (i <= kd) p[i & 1] = fma(lc[i], acc[(cc + i) & (PBM_RK - 1)], p[i & 1]);
                xj = (bj - (p[0] + p[1])) / lc[0];
                acc[cc] = xj;
              } else {
                T p0 = T(0), p1 = T(0), p2 = T(0), p3 = T(0);
                int slot = jm;
                auto next = [&]() {
                  slot = slot + 1 == w ? 0 : slot + 1;
                  return ring[slot * 64 + lane];
                };
                int i = 1;
                for (; i + 3 <= kd; i += 4) {
                  p0 = fma(lc[i], next(), p0);
                  p1 = fma(lc[i + 1], next(), p1);
                  p2 = fma(lc[i + 2], next(), p2);
                  p3 = fma(lc[i + 3], next(), p3);
                }
                for (; i <= kd; ++i) p0 = fma(lc[i], next(), p0);
                xj = (bj - ((p0 + p1) + (p2 + p3))) / lc[0];
                ring[jm * 64 + lane] = xj;              // (over row j + kd + 1, which no later column reads)
                jm = jm == 0 ? w - 1 : jm - 1;
              }
              *mine = xj;
            }
          }
        }
        band_lds_fence();
        park_L(lpre);
        band_lds_fence();
      }
      store_tile(dst, dst_perm, j0t);
      band_lds_fence();
      park_tile(tpre);
      band_lds_fence();
    }
  };

  using Fwd = std::integral_constant<bool, true>;
  using Bwd = std::integral_constant<bool, false>;
  if (which == 0) {
    sweep(Fwd{}, rhs, true, x, true);                   // y_j and then x_j live at x[perm[j]]
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // (the y other lanes of this wave stored)
    __builtin_amdgcn_wave_barrier();
    sweep(Bwd{}, x, true, x, true);
    return;
  }
  if (which == 2)
    sweep(Fwd{}, rhs, true, x, alias != 0);             // aliased: y_j stays at x[perm[j]] for now
  else
    sweep(Bwd{}, rhs, false, x, alias == 0);            // aliased: x_j stays at x[j] for now
  if (!alias) return;
  // the aliased call: each row moves into its output order through LDS (n elements, the launcher sized it)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
  __builtin_amdgcn_wave_barrier();
  T* stage = reinterpret_cast<T*>(pbm_smem);
  const int nv = min(64, nrhs - v0);
  for (int vec = 0; vec < nv; ++vec) {
    T* row = x + (int64_t)b * bstride + (int64_t)(v0 + vec) * ldv;
    band_lds_fence();
    for (int k = lane; k < n; k += 64) stage[k] = row[k];
    band_lds_fence();
    for (int k = lane; k < n; k += 64) {
      const int p = perm[k];
      if (which == 2)
        row[k] = stage[p];
      else
        row[p] = stage[k];
    }
  }
}

// ---- the band of the inverse -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// per-wave LDS elements: the window's torus and one chunk of Lb
__host__ __device__ inline size_t pbi_elems(int w, int S) { return (size_t)w * S + (size_t)BAND_CH * w; }

template <typename T>
__global__ __launch_bounds__(64 * BAND_WAVES) void pb_inverse_band_kernel(const T* __restrict__ Lb, int n, int kd, int B,
                                                                          T* __restrict__ Zb, int S) {
  extern __shared__ __attribute__((aligned(16))) char pbi_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;
  const int w = kd + 1;
  T* win = reinterpret_cast<T*>(pbi_smem) + (size_t)wave * pbi_elems(w, S);   // [w][S]: S(r, c) at [c mod w][r mod w]
  T* lst = win + w * S;                                                       // [CH][w]
  const T* Lo = Lb + (int64_t)b * n * w;
  T* Zo = Zb + (int64_t)b * n * w;
  const int64_t lmax = (int64_t)n * w - 1;
  const int nl = (BAND_CH * w + 63) >> 6;
  auto load_L = [&](int j0, T(&pre)[BAND_CH]) {
#pragma unroll
    for (int q = 0; q < BAND_CH; ++q)
      if (q < nl) {
        int64_t e = (int64_t)j0 * w + q * 64 + lane;
        e = e < 0 ? 0 : (e > lmax ? lmax : e);
        pre[q] = Lo[e];
      }
  };
  auto park_L = [&](const T(&pre)[BAND_CH]) {
#pragma unroll
    for (int q = 0; q < BAND_CH; ++q)
      if (q < nl && q * 64 + lane < BAND_CH * w) lst[q * 64 + lane] = pre[q];
  };
  T lpre[BAND_CH];
  const int jtop = (n - 1) & ~(BAND_CH - 1);
  load_L(jtop, lpre);
  for (int k = lane; k < w * S; k += 64) win[k] = T(0);   // rows and columns past n - 1: zero
  park_L(lpre);
  band_lds_fence();
  int jm = (n - 1) % w;
  for (int j0 = jtop; j0 >= 0; j0 -= BAND_CH) {
    load_L(j0 - BAND_CH, lpre);                           // (the next chunk, in flight under this one)
    for (int j = min(j0 + BAND_CH, n) - 1; j >= j0; --j) {
      const T* lc = lst + (j - j0) * w;
      const T rd = T(1) / lc[0];
      int ri = jm + lane;                                 // this lane's row j + i on the torus
      ri = ri >= w ? ri - w : ri;
      ri = lane <= kd ? ri : 0;
      const bool off = lane >= 1 && lane <= kd && j + lane < n;
      T p0 = T(0), p1 = T(0);
      int slot = jm;
      int k = 1;
      for (; k + 1 <= kd; k += 2) {
        slot = slot + 1 == w ? 0 : slot + 1;
        p0 = fma(lc[k], win[slot * S + ri], p0);
        slot = slot + 1 == w ? 0 : slot + 1;
        p1 = fma(lc[k + 1], win[slot * S + ri], p1);
      }
      if (k <= kd) {
        slot = slot + 1 == w ? 0 : slot + 1;
        p0 = fma(lc[k], win[slot * S + ri], p0);
      }
      const T z = off ? -rd * (p0 + p1) : T(0);
      const T dsum = wave_sum(off ? lc[min(lane, kd)] * z : T(0));
      const T zd = rd * rd - rd * dsum;
      const T v = lane == 0 ? zd : z;
      band_lds_fence();                                   // (every lane has read column and row j + kd + 1's slot)
      if (lane <= kd) {
        win[jm * S + ri] = v;
        win[ri * S + jm] = v;
        Zo[(int64_t)j * w + lane] = v;
      }
      band_lds_fence();
      jm = jm == 0 ? w - 1 : jm - 1;
    }
    park_L(lpre);
    band_lds_fence();
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <typename T>
int pb_solve_multi_impl(const void* Lb, int n, int kd, int B, const int32_t* perm, const void* rhs, void* x, int nrhs, int64_t ldv,
                        int64_t bstride, int which, hipStream_t st) {
  const char* who = "thx_pb_solve_multi";
  const bool reg = kd + 1 <= PBM_RK, alias = rhs == x && which != 0;
  size_t lds = pbm_elems(kd + 1, !reg) * sizeof(T);
  if (alias) {
    if ((size_t)n * sizeof(T) > BAND_LDS_BUDGET)
      return fail(who, ": with which = 1 or 2, x may alias rhs only up to 64 KB per vector (rows are permuted through LDS)");
    lds = lds > (size_t)n * sizeof(T) ? lds : (size_t)n * sizeof(T);
  }
  const int ngroups = (nrhs + 63) / 64;
  const dim3 grid((unsigned)((int64_t)B * ngroups)), block(64);
  if (reg)
    pb_solve_multi_kernel<T, true><<<grid, block, lds, st>>>(static_cast<const T*>(Lb), n, kd, ngroups, perm, static_cast<const T*>(rhs),
                                                             static_cast<T*>(x), nrhs, ldv, bstride, which, (int)alias);
  else
    pb_solve_multi_kernel<T, false><<<grid, block, lds, st>>>(static_cast<const T*>(Lb), n, kd, ngroups, perm,
                                                              static_cast<const T*>(rhs), static_cast<T*>(x), nrhs, ldv, bstride, which,
                                                              (int)alias);
  return check_launch(who);
}

template <typename T>
int pb_inverse_band_impl(const void* Lb, int n, int kd, int B, void* Zb, hipStream_t st) {
  const int w = kd + 1, S = w | 1;
  const size_t per_wave = pbi_elems(w, S) * sizeof(T);
  int waves = (int)(BAND_LDS_BUDGET / per_wave);
  waves = waves < 1 ? 1 : (waves > BAND_WAVES ? BAND_WAVES : waves);
  const unsigned grid = (unsigned)((B + waves - 1) / waves);
  pb_inverse_band_kernel<T><<<dim3(grid), dim3(64 * waves), per_wave * waves, st>>>(static_cast<const T*>(Lb), n, kd, B,
                                                                                   static_cast<T*>(Zb), S);
  return check_launch("thx_pb_inverse_band");
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_pb_solve_multi(const void* Lb, int32_t n, int32_t kd, int32_t B, const int32_t* perm, const void* rhs, void* x, int32_t nrhs,
                       int64_t ldv, int64_t bstride, int which, int dtype, void* stream) {
  const char* who = "thx_pb_solve_multi";
  if (!Lb || !perm || !rhs || !x) return fail(who, ": null pointer");
  if (int r = check_band_sizes(who, n, kd, B)) return r;
  if (nrhs < 1) return fail(who, ": nrhs < 1");
  if (ldv < n) return fail(who, ": ldv < n");
  if (bstride / nrhs < ldv) return fail(who, ": bstride < nrhs * ldv");   // (no product: nrhs * ldv may not fit)
  if (which < 0 || which > 2) return fail(who, ": which = 0 (both), 1 (backward only), 2 (forward only)");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if ((int64_t)B * (((int64_t)nrhs + 63) / 64) > 0x7fffffffLL) return fail(who, ": B * ceil(nrhs / 64) exceeds the grid limit");
  THX_DISPATCH(dtype, return pb_solve_multi_impl<float>(Lb, n, kd, B, perm, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)),
               return pb_solve_multi_impl<double>(Lb, n, kd, B, perm, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)));
  return 0;
}

int thx_pb_inverse_band(const void* Lb, int32_t n, int32_t kd, int32_t B, void* Zb, int dtype, void* stream) {
  const char* who = "thx_pb_inverse_band";
  if (!Lb || !Zb) return fail(who, ": null pointer");
  if (int r = check_band_sizes(who, n, kd, B)) return r;
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (Lb == Zb) return fail(who, ": Zb must not alias Lb (columns of Lb are read after the same columns of Zb are written)");
  THX_DISPATCH(dtype, return pb_inverse_band_impl<float>(Lb, n, kd, B, Zb, as_stream(stream)),
               return pb_inverse_band_impl<double>(Lb, n, kd, B, Zb, as_stream(stream)));
  return 0;
}

}  // extern "C"
