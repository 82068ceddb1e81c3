#pragma once
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_engine.cuh"
#include "chol_potrf.cuh"
#include "chol_tiles.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// chol_diag: SYRK + blocked Cholesky of the 128x128 diagonal tile of block column j, panel M_j,
// fused forward substitution
// ------------------------------------------------------------------------------------------------
template <typename T>
struct DiagSmem {
  // ten 32 x LDB sub-blocks; the K-loop's staging buffer (128 x SYRK_LDT) lives in its head
  static constexpr size_t tile = (size_t)10 * 32 * CT<T>::LDB * sizeof(T);
  static_assert(10 * 32 * CT<T>::LDB >= Engine<T>::SYRK_STAGE, "staging buffer must fit in the tile");
  // tile | vvec [128] T | ubuf [32] T | ybuf [ypad] T
  static size_t bytes(int ypad) { return tile + 160 * sizeof(T) + (size_t)ypad * sizeof(T); }
};

template <typename T, bool HB>
__global__ void __launch_bounds__(256, sizeof(T) == 4 ? 3 : 1)
chol_diag_kernel(const T* __restrict__ H, T* __restrict__ L, T* __restrict__ panel, const T* __restrict__ damping,
                 int ellipsoidal, T damping_eps, int32_t* __restrict__ info, int n, int64_t ld, int j0, int ntiles,
                 const T* __restrict__ rhs, T* __restrict__ yout, int64_t ldv, TilePat pat, HBlk hb) {
  using C = CT<T>;
  using V = typename C::V;
  using E = Engine<T>;
  const int j = j0 + blockIdx.y;   // (level schedule: blockIdx.y runs over the level's block columns)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);  // lower sub-blocks (tblk); its head doubles as the K-loop staging buffer
  T* vvec = reinterpret_cast<T*>(smem_raw + DiagSmem<T>::tile);
  T* ubuf = vvec + 128;
  T* ybuf = ubuf + 32;
  const int b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const LFrame lf = lframe(pat, ld);
  const int64_t mat = (int64_t)b * ld * ld;            // H: always the dense frame (or the block list)
  const int64_t lmat = (int64_t)b * lf.pstride;        // L: dense frame or tile-packed
  const int64_t ldt = lf.ld;
  T* const Ljj = L + lmat + lf.tile(j, j, j);          // the diagonal tile of L
  const int row0 = j * TILE;
  const int valid = tile_rows(pat, n, j);

  const bool fwd = rhs != nullptr;

  // SYRK on the 36 lower 16x16 blocks of the tile, nine per wave (Engine<T>::syrk36)
  // tile-sparse: only the block columns k < j in which row panel j is non-zero
  const int32_t* klist = pat.diag_k ? pat.diag_k + pat.diag_kptr[j] : nullptr;
  const int Kspan = pat.rl ? (pat.rl_la ? TILE : 0) : (pat.diag_k ? (pat.diag_kptr[j + 1] - pat.diag_kptr[j]) * TILE : row0);
  const int kcol0 = (pat.rl && pat.rl_la) ? (j - 1) * TILE : 0;   // (right-looking look-ahead: the K-loop is the one tile L_j,j-1)
  const bool ycompact = pat.ent_col != nullptr;   // (level schedule: ybuf holds the K-list's blocks of y only)
  typename E::Sy acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = T(0);
  T tpart = T(0);  // this thread's half of (L_j,0:j y)[tid >> 1]
  std::conditional_t<sizeof(T) == 4, float4, f64x4> hpre[9];
  // issued behind the loads of the first k-chunk (kloop_f's after_issue hook): y_0:j of the earlier columns -> LDS, and the
  // H_jj blocks, in flight during the whole K-loop
  HBPre<T, HB ? HB_NPRE_DIAG : 1> hbp;
  auto prologue = [&]() __attribute__((always_inline)) {
    if (fwd) {
      if (ycompact) {   // level schedule: the blocks of y this column's K-list names, back to back
        for (int k = tid; k < Kspan; k += 256) ybuf[k] = yout[(int64_t)b * ldv + klist[k >> 7] * TILE + (k & (TILE - 1))];
      } else {
        for (int k = tid; k < row0; k += 256) ybuf[k] = yout[(int64_t)b * ldv + k];
      }
    }
    if constexpr (!HB) {
      const T* Hjj = H + mat + (int64_t)row0 * ld + row0;
      if (wave == 0) E::template syrk36_prefetch<0>(Hjj, ld, valid, hpre, lane);
      else if (wave == 1) E::template syrk36_prefetch<1>(Hjj, ld, valid, hpre, lane);
      else if (wave == 2) E::template syrk36_prefetch<2>(Hjj, ld, valid, hpre, lane);
      else E::template syrk36_prefetch<3>(Hjj, ld, valid, hpre, lane);
    } else {   // block-compact H: the tile's blocks are ADDED after the SYRK (below); the "H" of the store is zero
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<T*>(&hpre[i])[k] = T(0);
      hbp.load(hb, b, j, j, tid);
    }
  };
  kloop_f<T, true, true, E::SYRK_LDT, (sizeof(T) == 8 && CT<T>::KB == 32)>(
      L + lmat + (lf.packed ? 0 : (int64_t)row0 * ld) + kcol0, valid, nullptr, 0, ldt, Kspan, tile, nullptr, tid,
      (fwd && !pat.rl) ? ybuf : nullptr, &tpart, [&]() __attribute__((always_inline)) {
    if (wave == 0) E::template syrk36<0>(tile, acc, lane);
    else if (wave == 1) E::template syrk36<1>(tile, acc, lane);
    else if (wave == 2) E::template syrk36<2>(tile, acc, lane);
    else E::template syrk36<3>(tile, acc, lane);
  },
  prologue, klist, lf.packed ? pat.diag_s + pat.diag_kptr[j] : nullptr, nullptr, lf.pstride, ycompact);

  // ---- S = H_jj (+ damping on the diagonal) - acc -> LDS tile; identity padding outside the matrix ----
  __syncthreads();  // staging buffer is free
  if (tid < TILE) vvec[tid] = (fwd && tid < valid) ? rhs[(int64_t)b * ldv + row0 + tid] : T(0);
  {
    const bool damp = damping != nullptr;
    const T lam = damp ? damping[b] : T(0);
    const bool sd = damp && !HB;   // (block-compact H: the damping rides on the diagonal elements of the gathered blocks)
    if (wave == 0) E::template syrk36_store<0>(tile, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else if (wave == 1) E::template syrk36_store<1>(tile, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else if (wave == 2) E::template syrk36_store<2>(tile, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else E::template syrk36_store<3>(tile, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    __syncthreads();  // vvec visible
    {  // g_j - L_j,0:j y : thread pair (2r, 2r+1) holds the two halves of row r's sum
      const T tsum = tpart + __shfl_xor(tpart, 1);
      if (fwd && (tid & 1) == 0) vvec[tid >> 1] -= tsum;
    }
    if constexpr (HB) {   // S += H_jj (+ damping): each element of the tile's lower triangle belongs to at most one piece
      hbp.foreach(hb, b, tid, [&](int r, int c, T v) __attribute__((always_inline)) {
        if (c > r) return;
        if (r == c && damp) v = ellipsoidal ? v + (lam * v + damping_eps) : v + lam;
        tile[tblk<T>(r >> 5, c >> 5) + (r & 31) * C::LDB + (c & 31)] += v;
      });
    }
  }
  __syncthreads();

  // ---- blocked right-looking Cholesky on the LDS tile, 32-wide sub-blocks.  Afterwards the tile IS the
  //      solve panel: W_ss = L_ss^-1 on the diagonal sub-blocks, -L_us below them. ----
  for (int sb = 0; sb < 4; ++sb) {
    T* Dss = tile + tblk<T>(sb, sb);
    if (wave == 0) {
      const int bad = potrf_inv32<T>(Dss, Ljj + (int64_t)(32 * sb) * ldt + 32 * sb, ldt, valid - 32 * sb, lane);
      if (bad != 0 && lane == 0 && info[b] == 0) info[b] = row0 + 32 * sb + bad;
    }
    __syncthreads();
    if (sb == 3) break;
    // L_us = S_us W_ss^T for the sub-blocks below (one per wave), stored negated
    {
      const int u = sb + 1 + wave;
      if (u < 4) {
        T* Dus = tile + tblk<T>(u, sb);
        typename E::Blk X;
        E::blk_zero(X);
        E::blk_mma(Dss, Dus, X, lane, T(1));
        E::blk_store(X, Dus, lane, T(-1));
      }
    }
    __syncthreads();
    // trailing update S_uv -= L_us L_vs^T, sb < v <= u: blocks dealt round-robin to the waves
    {
      int idx = 0;
      for (int u = sb + 1; u < 4; ++u)
        for (int v = sb + 1; v <= u; ++v, ++idx) {
          if ((idx & 3) != wave) continue;
          T* Duv = tile + tblk<T>(u, v);
          typename E::Blk D;
          E::blk_load(D, Duv, lane);
          // tile(v,s) = -L_vs is negated on load, tile(u,s) = -L_us:  D += (+L_vs)(-L_us)^T
          E::blk_mma(tile + tblk<T>(v, sb), tile + tblk<T>(u, sb), D, lane, T(-1));
          E::blk_store(D, Duv, lane, T(1));
        }
    }
    __syncthreads();
  }

  // ---- outputs: strictly-lower sub-blocks of L_jj (= -tile), the panel, y_j ----
  {  // (the panel's sub-blocks above the diagonal are never read -- chol_offdiag and the solves use the lower ten -- and
     //  are not written)
    constexpr int VPR = 32 / C::VEC;  // vectors per sub-block row
    T* Lt = Ljj;
    T* P = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
    for (int u = 0; u < 4; ++u)
      for (int v = 0; v <= u; ++v) {
        const T* blk = tile + tblk<T>(u, v);
#pragma unroll
        for (int idx = tid; idx < 32 * VPR; idx += 256) {
          const int rr = idx / VPR, c = (idx % VPR) * C::VEC;
          const V val = *reinterpret_cast<const V*>(blk + rr * C::LDB + c);
          *reinterpret_cast<V*>(P + (32 * u + rr) * TILE + 32 * v + c) = val;
          if (u > v && 32 * u + rr < valid) {
            V* dst = reinterpret_cast<V*>(Lt + (int64_t)(32 * u + rr) * ldt + 32 * v + c);
            if constexpr (sizeof(T) == 4) *dst = make_float4(-val.x, -val.y, -val.z, -val.w);
            else *dst = make_double2(-val.x, -val.y);
          }
        }
      }
  }
  if (fwd) {
    if (wave == 0) {   // (the shared column-by-column substitution: same rounding as chol_potrf_kernel's)
      for (int sb = 0; sb < 4; ++sb) {
        typename E::Blk Wb;
        E::blk_load(Wb, tile + tblk<T>(sb, sb), lane);
        fwd_diag_block<T>(Wb, vvec, sb, lane);
        for (int u = sb + 1; u < 4; ++u) {
          typename E::Blk Xb;
          E::blk_load(Xb, tile + tblk<T>(u, sb), lane);
          fwd_below_block<T>(Xb, vvec, sb, u, lane);
        }
        wave_lds_fence();
      }
    }
    __syncthreads();
    if (tid < valid) yout[(int64_t)b * ldv + row0 + tid] = vvec[tid];
  }
}

// ------------------------------------------------------------------------------------------------
// The diagonal phase SPLIT in two kernels:
//   chol_syrk_kernel : the MFMA half of chol_diag -- S = H_jj + damping - L_j,0:j L_j,0:j^T (36 lower 16x16 blocks, nine per wave),
//                      riding on it g_j - L_j,0:j y -- written to the diagonal tile's place in the global factor / to y_j.
//                      No serial phase: all four waves of all three resident workgroups issue MFMAs for the kernel's whole life.
//   chol_potrf_kernel: the serial half, ONE WAVE per tile.  The tile's ten lower 32x32 sub-blocks live in that wave's registers in
//                      the MFMA C/D layout (160 VGPRs in fp32); the sub-block TRSMs and trailing updates are register x register
//                      MFMAs (Engine::blk_mma_rr: no LDS traffic at all), only the 32x32 diagonal sub-block being factorised and
//                      inverted passes through a 4.6 KB LDS block (potrf_inv32).  5 KB of LDS and <= 256 VGPRs per tile:
//                      EIGHT tiles per CU are in their latency-bound pivot chains at once, against three with chol_diag -- whose
//                      workgroup pinned 53 KB of LDS and three idle waves' registers for the 126 k cycles of its chain, i.e. kept
//                      a third of a CU from anything else.
// ------------------------------------------------------------------------------------------------
template <typename T>
struct SyrkSmem {
  static size_t bytes(int ypad) { return (size_t)Engine<T>::SYRK_STAGE * sizeof(T) + (size_t)ypad * sizeof(T); }
};

constexpr int SYRK32_WAVES = 3;
// waves per SIMD the fp64 block-compact SYRK is compiled for: 3 (168 VGPRs + 20 B of scratch) instead of 2 (200 VGPRs) takes 0.7 ms
// off the headline factorisation (87.9 / 88.0 -> 87.2 / 87.3 ms: its short K-loops want a third workgroup per CU); 4 (128 VGPRs,
// 168 B of scratch) costs 2.7 ms (profiles/r6/ag_)
constexpr int SYRK64_WAVES = 3;
// SORTED ROWS (SR; FactorPlan.sortrows, HBlk.tr_perm16 / tr_mask16; fp32, block-compact H, dense frame, left-looking): the tile's 128
// rows are staged in the order tr_perm16[j] -- sorted by their first non-zero column, sixteen to a block row -- and tr_mask16[j][kc]
// names the block rows that have begun at k-chunk kc.  For the others the loads, the staging stores and every product with them
// are left out; each element keeps its products in their order.  Behind the K-loop the staged lower triangle goes back to
// natural order through LDS (SYRK_SR_TRI floats, over the staging buffer and y), and everything else runs as without it.
constexpr int SYRK_SR_TRI = TILE * (TILE + 1) / 2;
// workgroups per CU the SR instantiation is compiled for.  The natural-order fp32 block-compact instance needs 128 VGPRs under
// SYRK32_WAVES, so FOUR of its workgroups fit a CU; SR is held to the same 128 (no scratch).  Left at SYRK32_WAVES and with a
// straight-line path for fully active chunks it took 145 VGPRs, three per CU, and the factor 35.19 - 35.23 ms instead of
// 34.83 - 34.97 (profiles/tile_sorted_rows/variant_three_per_cu.txt, bench_first_set.txt).
constexpr int SYRK32_SR_WAVES = 4;
static_assert(SYRK32_SR_WAVES >= SYRK32_WAVES, "never fewer workgroups per CU than the natural-order instance is compiled for");
template <typename T, bool HB, bool SR = false>
__global__ void __launch_bounds__(256, sizeof(T) == 4 ? (HB ? (SR ? SYRK32_SR_WAVES : SYRK32_WAVES) : 3) : (HB ? SYRK64_WAVES : 2))
chol_syrk_kernel(const T* __restrict__ H, T* __restrict__ L, const T* __restrict__ damping, int ellipsoidal, T damping_eps,
                 int n, int64_t ld, int j0, const T* __restrict__ rhs, T* __restrict__ yout, int64_t ldv, TilePat pat, HBlk hb) {
  using E = Engine<T>;
  const int j = j0 + blockIdx.y;   // (level schedule: blockIdx.y runs over the level's block columns)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* stage = reinterpret_cast<T*>(smem_raw);                 // K-loop staging buffer, 128 x SYRK_LDT
  T* ybuf = stage + E::SYRK_STAGE;                           // y_0:j of the earlier columns
  const int b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const LFrame lf = lframe(pat, ld);
  const int64_t mat = (int64_t)b * ld * ld;            // H (dense frame)
  const int64_t lmat = (int64_t)b * lf.pstride;        // L (dense frame or tile-packed)
  const int64_t ldt = lf.ld;
  const int row0 = j * TILE;
  const int valid = tile_rows(pat, n, j);
  const bool fwd = rhs != nullptr;

  // tile-sparse: only the block columns k < j in which row panel j is non-zero
  const int32_t* klist = pat.diag_k ? pat.diag_k + pat.diag_kptr[j] : nullptr;
  const int Kspan = pat.diag_k ? (pat.diag_kptr[j + 1] - pat.diag_kptr[j]) * TILE : row0;
  const bool ycompact = pat.ent_col != nullptr;   // (level schedule: ybuf holds the K-list's blocks of y only)
  typename E::Sy acc[9];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[i][k] = T(0);
  T tpart = T(0);  // this thread's half of (L_j,0:j y)[tid >> 1]
  std::conditional_t<sizeof(T) == 4, float4, f64x4> hpre[9];
  HBPre<T, HB ? HB_NPRE_DIAG : 1> hbp;
  auto prologue = [&]() __attribute__((always_inline)) {
    if (fwd) {
      if (ycompact) {   // level schedule: the blocks of y this column's K-list names, back to back
        for (int k = tid; k < Kspan; k += 256) ybuf[k] = yout[(int64_t)b * ldv + klist[k >> 7] * TILE + (k & (TILE - 1))];
      } else {
        for (int k = tid; k < row0; k += 256) ybuf[k] = yout[(int64_t)b * ldv + k];
      }
    }
    if constexpr (!HB) {
      const T* Hjj = H + mat + (int64_t)row0 * ld + row0;
      if (wave == 0) E::template syrk36_prefetch<0>(Hjj, ld, valid, hpre, lane);
      else if (wave == 1) E::template syrk36_prefetch<1>(Hjj, ld, valid, hpre, lane);
      else if (wave == 2) E::template syrk36_prefetch<2>(Hjj, ld, valid, hpre, lane);
      else E::template syrk36_prefetch<3>(Hjj, ld, valid, hpre, lane);
    } else {   // block-compact H: the tile's blocks are ADDED after the SYRK (below); the "H" of the store is zero
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) reinterpret_cast<T*>(&hpre[i])[k] = T(0);
      hbp.load(hb, b, j, j, tid);
    }
  };
  [[maybe_unused]] int srow = tid >> 1;   // the tile's row whose forward-substitution sum this thread pair holds
  if constexpr (SR) {
    static_assert(sizeof(T) == 4 && HB, "sorted rows: fp32, block-compact H");
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const int32_t __attribute__((address_space(4))) * cmask_t;
    const int32_t* perm = hb.tr_perm16 + j * TILE;
    const cmask_t pm = (cmask_t)(uintptr_t)(hb.tr_mask16 + (int64_t)j * 4 * ((n + TILE - 1) / TILE));
    // staged row lrow + 32 u of pass u lies in block row 2 u + hi: wave uniform
    const int lrow = tid >> 3, lc = tid & 7, hi = __builtin_amdgcn_readfirstlane(wave >> 1);
    unsigned voff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) voff[u] = (unsigned)((perm[lrow + 32 * u] * (int)ld + lc * 4) * 4);
    // (rows behind the matrix: outside the buffer's extent, read as zeros)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(L + lmat + (int64_t)row0 * ld), 0,
                                                                          (int)((int64_t)valid * ld * 4), 0x00020000);
    const int nk = Kspan / 32;
    uint4 ra[2][4];   // (a piece is loaded and staged under the same mask bit)
    auto gload = [&](uint4 (&x)[4], int kc, int m) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((m >> (2 * u + hi)) & 1) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff[u], kc * 128, 0);
          x[u] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    // the masks of chunks kc .. kc + 3: the prefetch two chunks ahead branches on m2, and m3 was asked for a chunk before that
    int m0 = pm[0], m1 = nk > 1 ? pm[1] : 0, m2 = nk > 2 ? pm[2] : 0, m3 = nk > 3 ? pm[3] : 0;
    gload(ra[0], 0, m0);
    if (nk > 1) gload(ra[1], 1, m1);
    prologue();
    T gsum = T(0);
    auto step = [&](uint4 (&x)[4], int kc) __attribute__((always_inline)) {
      const int mc = m0;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((mc >> (2 * u + hi)) & 1) *reinterpret_cast<uint4*>(stage + (lrow + 32 * u) * E::SYRK_LDT + 4 * lc) = x[u];
      __syncthreads();
      if (kc + 2 < nk) gload(x, kc + 2, m2);
      m0 = m1, m1 = m2, m2 = m3;
      m3 = kc + 4 < nk ? pm[kc + 4] : 0;
      if (fwd && ((mc >> (tid >> 5)) & 1)) {   // staged slot tid >> 1 lies in block row tid >> 5
        const float4* rp = reinterpret_cast<const float4*>(stage + (tid >> 1) * E::SYRK_LDT + (tid & 1) * 16);
        const float4* yp = reinterpret_cast<const float4*>(ybuf + kc * 32 + (tid & 1) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 a = rp[i], yv = yp[i];
          gsum += a.x * yv.x; gsum += a.y * yv.y; gsum += a.z * yv.z; gsum += a.w * yv.w;
        }
      }
      if (wave == 0) E::template syrk36_masked<0>(stage, acc, lane, mc);
      else if (wave == 1) E::template syrk36_masked<1>(stage, acc, lane, mc);
      else if (wave == 2) E::template syrk36_masked<2>(stage, acc, lane, mc);
      else E::template syrk36_masked<3>(stage, acc, lane, mc);
    };
    for (int kc = 0; kc < nk; kc += 2) {
      step(ra[0], kc);
      if (kc + 1 < nk) step(ra[1], kc + 1);
    }
    tpart = gsum;
    srow = perm[tid >> 1];
    // staged element (s, t) -> natural element (max, min) of (perm[s], perm[t]) of the packed lower triangle in LDS; of a diagonal
    // block's two equal halves only s >= t is written; then every lane reads its natural fragments back (an element above the
    // diagonal as its mirror image, which is what the natural-order accumulators hold there)
    __syncthreads();   // the staging buffer and y are free
    T* tri = stage;
    auto put = [&](int u, int v, const f32x4& a) __attribute__((always_inline)) {
      const int s = 16 * u + (lane & 15), t0 = 16 * v + 4 * (lane >> 4);
      const int ps = perm[s];
      const int4 pt = *reinterpret_cast<const int4*>(perm + t0);
      const int ptk[4] = {pt.x, pt.y, pt.z, pt.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int hi_ = max(ps, ptk[k]), lo_ = min(ps, ptk[k]);
        if (u != v || s >= t0 + k) tri[hi_ * (hi_ + 1) / 2 + lo_] = a[k];
      }
    };
    auto get = [&](int u, int v, f32x4& a) __attribute__((always_inline)) {
      const int r = 16 * u + (lane & 15), c0 = 16 * v + 4 * (lane >> 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int hi_ = max(r, c0 + k), lo_ = min(r, c0 + k);
        a[k] = tri[hi_ * (hi_ + 1) / 2 + lo_];
      }
    };
    const int UH = 4 + wave, UL = 3 - wave;
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if (i <= UH) put(UH, i, acc[i]);
      else put(UL, i - UH - 1, acc[i]);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 9; ++i)
      if (i <= UH) get(UH, i, acc[i]);
      else get(UL, i - UH - 1, acc[i]);
  } else {
  kloop_f<T, true, true, E::SYRK_LDT, (sizeof(T) == 8 && CT<T>::KB == 32)>(
      L + lmat + (lf.packed ? 0 : (int64_t)row0 * ld), valid, nullptr, 0, ldt, Kspan, stage, nullptr, tid,
      fwd ? ybuf : nullptr, &tpart, [&]() __attribute__((always_inline)) {
    if (wave == 0) E::template syrk36<0>(stage, acc, lane);
    else if (wave == 1) E::template syrk36<1>(stage, acc, lane);
    else if (wave == 2) E::template syrk36<2>(stage, acc, lane);
    else E::template syrk36<3>(stage, acc, lane);
  }, prologue, klist, lf.packed ? pat.diag_s + pat.diag_kptr[j] : nullptr, nullptr, lf.pstride, ycompact);
  }

  {
    const bool damp = damping != nullptr;
    const T lam = damp ? damping[b] : T(0);
    T* Lt = L + lmat + lf.tile(j, j, j);
    const bool sd = damp && !HB;
    if (wave == 0) E::template syrk36_store_global<0>(Lt, ldt, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else if (wave == 1) E::template syrk36_store_global<1>(Lt, ldt, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else if (wave == 2) E::template syrk36_store_global<2>(Lt, ldt, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    else E::template syrk36_store_global<3>(Lt, ldt, hpre, acc, lane, valid, sd, lam, ellipsoidal, damping_eps);
    if constexpr (HB) {
      // block-compact H: the tile now holds -L_j L_j^T; its pieces of H (+ damping on the diagonal) are added in place.  The
      // stores above are this workgroup's own: visible to all its threads after the fence + barrier.
      __threadfence_block();
      __syncthreads();
      hbp.foreach(hb, b, tid, [&](int r, int c, T v) __attribute__((always_inline)) {
        if (c > r || r >= valid) return;
        if (r == c && damp) v = ellipsoidal ? v + (lam * v + damping_eps) : v + lam;
        Lt[(int64_t)r * ldt + c] += v;
      });
    }
  }
  if (fwd) {  // g_j - L_j,0:j y -> y_j's place (chol_potrf_kernel finishes it): thread pair (2r, 2r+1) holds the halves of row r
    const T tsum = tpart + __shfl_xor(tpart, 1);
    const int r = SR ? srow : tid >> 1;   // (SR: the pair holds a staged slot's sum)
    if ((tid & 1) == 0 && r < valid) yout[(int64_t)b * ldv + row0 + r] = rhs[(int64_t)b * ldv + row0 + r] - tsum;
  }
}

__device__ __forceinline__ constexpr int bidx(int u, int v) { return u * (u + 1) / 2 + v; }

constexpr int POTRF_F64_WAVES_PER_SIMD = 1;   // (2 = at most 256 registers: the compiler spills the rest to scratch)
template <typename T>
__global__ void __launch_bounds__(64, sizeof(T) == 4 ? 2 : POTRF_F64_WAVES_PER_SIMD)
chol_potrf_kernel(T* __restrict__ L, T* __restrict__ panel, int32_t* __restrict__ info, int n, int64_t pstride, int64_t tile_off0,
                  int64_t ld, int j0, int ntiles, T* __restrict__ yout, int64_t ldv, const int32_t* __restrict__ tile_valid) {
  // (the diagonal tile of problem b starts at L + b * pstride + tile_off, row stride ld: dense frame or tile-packed factor;
  //  level schedule -- tile-packed factor only -- blockIdx.y runs over the level's block columns: slot j0 + blockIdx.y)
  const int j = j0 + blockIdx.y;
  const int64_t tile_off = tile_off0 + (int64_t)blockIdx.y * TILE * TILE;
  using C = CT<T>;
  using E = Engine<T>;
  using Blk = typename E::Blk;
  __shared__ __attribute__((aligned(16))) T Dss[32 * C::LDB];   // the diagonal sub-block being factorised / inverted
  __shared__ __attribute__((aligned(16))) T vvec[TILE];         // right-hand side / solution of the fused forward substitution
  // fp32, two waves per SIMD (256 VGPRs): while the FIRST diagonal sub-block is factorised -- nine other sub-blocks live next to
  // the temporaries of potrf_inv32 -- the last block row waits in LDS instead of in spilled registers
  constexpr int PARK = sizeof(T) == 4 ? 3 : 0;
  __shared__ __attribute__((aligned(16))) T park[PARK > 0 ? PARK * 32 * C::LDB : 4];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int row0 = j * TILE, valid = tile_valid ? tile_valid[j] : min(TILE, n - row0);
  T* Lt = L + (int64_t)b * pstride + tile_off;
  const bool fwd = yout != nullptr;

  // the tile: S (written by chol_syrk_kernel) -> registers; identity outside the matrix
  Blk Tb[10];
  static_for<4>([&](auto iu) __attribute__((always_inline)) {
    constexpr int u = decltype(iu)::value;
    static_for<u + 1>([&](auto iv) __attribute__((always_inline)) {
      constexpr int v = decltype(iv)::value;
      E::blk_load_global(Tb[bidx(u, v)], Lt + (int64_t)(32 * u) * ld + 32 * v, Lt, ld, valid - 32 * u, valid - 32 * v, u == v, lane);
    });
  });
  if (fwd) {
#pragma unroll
    for (int k = lane; k < TILE; k += 64) vvec[k] = k < valid ? yout[(int64_t)b * ldv + row0 + k] : T(0);
  }

  // blocked right-looking Cholesky over the four 32-wide sub-block columns.  A finished column -- W_ss = L_ss^-1 on the diagonal
  // sub-block, -L_us below it: the solve panel's column -- is used at once for the fused forward substitution and stored, so
  // its registers are free for the rest of the factorisation.
  T* P = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
  static_for<4>([&](auto isb) __attribute__((always_inline)) {
    constexpr int sb = decltype(isb)::value;
    E::blk_store(Tb[bidx(sb, sb)], Dss, lane, T(1));
    if constexpr (sb == 0 && PARK > 0) {
      static_for<PARK>([&](auto ik) __attribute__((always_inline)) {
        constexpr int k = decltype(ik)::value;
        E::blk_store(Tb[bidx(3, 1 + k)], park + k * 32 * C::LDB, lane, T(1));
      });
    }
    wave_lds_fence();
    const int bad = potrf_inv32<T>(Dss, Lt + (int64_t)(32 * sb) * ld + 32 * sb, ld, valid - 32 * sb, lane);
    if (bad != 0 && lane == 0 && info[b] == 0) info[b] = row0 + 32 * sb + bad;
    wave_lds_fence();
    E::blk_load(Tb[bidx(sb, sb)], Dss, lane);   // W_ss (full 32 x 32, zero above the diagonal)
    if constexpr (sb == 0 && PARK > 0) {
      static_for<PARK>([&](auto ik) __attribute__((always_inline)) {
        constexpr int k = decltype(ik)::value;
        E::blk_load(Tb[bidx(3, 1 + k)], park + k * 32 * C::LDB, lane);
      });
    }
    E::blk_store_global(Tb[bidx(sb, sb)], P + (32 * sb) * TILE + 32 * sb, TILE, 32, lane, T(1));
    if (fwd) fwd_diag_block<T>(Tb[bidx(sb, sb)], vvec, sb, lane);   // y_s = W_ss u_s (u_s: what the earlier columns left)
    // L_us = S_us W_ss^T for the sub-blocks below, kept negated; u_u += (-L_us) y_s
    static_for<3 - sb>([&](auto iu) __attribute__((always_inline)) {
      constexpr int u = sb + 1 + decltype(iu)::value;
      Blk X;
      E::blk_zero(X);
      E::blk_mma_rr(Tb[bidx(sb, sb)], Tb[bidx(u, sb)], X, T(1));
      E::blk_neg(X);
      Tb[bidx(u, sb)] = X;
      E::blk_store_global(X, P + (32 * u) * TILE + 32 * sb, TILE, 32, lane, T(1));
      E::blk_store_global(X, Lt + (int64_t)(32 * u) * ld + 32 * sb, ld, valid - 32 * u, lane, T(-1));
      if (fwd) fwd_below_block<T>(X, vvec, sb, u, lane);
    });
    // trailing update S_uv -= L_us L_vs^T, sb < v <= u  (Tb(v,sb) = -L_vs is negated back, Tb(u,sb) = -L_us)
    static_for<3 - sb>([&](auto iu) __attribute__((always_inline)) {
      constexpr int u = sb + 1 + decltype(iu)::value;
      static_for<u - sb>([&](auto iv) __attribute__((always_inline)) {
        constexpr int v = sb + 1 + decltype(iv)::value;
        E::blk_mma_rr(Tb[bidx(v, sb)], Tb[bidx(u, sb)], Tb[bidx(u, v)], T(-1));
      });
    });
    if (fwd) wave_lds_fence();   // the vvec updates of this column before the next column reads them
  });
  if (fwd) {
#pragma unroll
    for (int k = lane; k < TILE; k += 64)
      if (k < valid) yout[(int64_t)b * ldv + row0 + k] = vvec[k];
  }
}

}  // namespace thx
