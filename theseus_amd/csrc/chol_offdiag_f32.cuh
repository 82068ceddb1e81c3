#pragma once
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_engine.cuh"
#include "chol_tiles.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// chol_offdiag: GEMM K-loop + blocked MFMA substitution  L_ij = (H_ij - sum) L_jj^-T.
// Two kernels, one per dtype; both keep two workgroups per CU resident and move H / the result between global memory and
// registers directly.  (The first version of this kernel staged H, the full 128x130 panel and the result through one LDS
// tile: 67 / 133 KB, every load phase exposed; it is gone.)
// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// chol_offdiag, fp32.  Nothing of the epilogue waits on memory: the H tile is prefetched into registers in the accumulator layout and the ten
// lower sub-blocks of the panel (40 KB, XOR-swizzled so that unpadded 32x32 blocks read conflict
// free) are copied to LDS BEFORE the K-loop; the result is stored straight from the registers.
// LDS: staging 36 KB + panel 40 KB -> two workgroups per CU.
// ------------------------------------------------------------------------------------------------
constexpr int OFF32_STAGE_FLOATS = 2 * 128 * 36;
constexpr int OFF32_SMEM = (OFF32_STAGE_FLOATS + 10 * 1024) * 4;

// D.block(S) += Pc[block (S,Tt)] * Bs.block(Tt)^T with the swizzled compact panel, i.e. for every tile row r this wave
// owns:  D[r][32S + i] += sum_{c in block Tt} M[32S + i][c] * Bs[r][c].  The B operand is the accumulator itself: an MFMA's
// k index is only a pairing of columns (k = 0/1 <-> columns c and c+4 held by lane groups 0/1).
template <int S, int Tt>
__device__ __forceinline__ void sub_mma_sw(const float* Pc, const Engine<float>::Acc& Bs, Engine<float>::Acc& D,
                                           int lane) {
  const int rl = lane & 31, g = lane >> 5;
  const float* brow = Pc + (S * (S + 1) / 2 + Tt) * 1024 + rl * 32;
  const int sw = (rl >> 1) & 7;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 fa = *reinterpret_cast<const float4*>(brow + (((2 * q + g) ^ sw) << 2));
    D.v[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, Bs.v[Tt][4 * q + 0], D.v[S], 0, 0, 0);
    D.v[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, Bs.v[Tt][4 * q + 1], D.v[S], 0, 0, 0);
    D.v[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, Bs.v[Tt][4 * q + 2], D.v[S], 0, 0, 0);
    D.v[S] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, Bs.v[Tt][4 * q + 3], D.v[S], 0, 0, 0);
  }
}

// SORTED COLUMNS of a HEAD tile (SC; FactorPlan.sorthead, HBlk.th_*; launched only for tile (j + 1, j) of the column-pair schedule
// when tile j has a table): the one-tile version of chol_offdiag2_f32_kernel<HB, true, true>.  Operand A -- the 128 rows of tile
// j -- is staged in the order th_perm32[j], four blocks of 32 sorted by first non-zero column; th_mask32[j][kc] names the blocks
// that have begun, the loads, staging stores and MFMAs of the others are left out (workgroup uniform), and the K-loop starts at
// th_k0h[j].  Every column accumulates independently and keeps its products in their order.  Behind the K-loop each wave moves its
// own 32 rows back to natural column order through its quarter of the staging buffers (the panel copy is already in LDS behind
// them): two rounds of 64 natural columns, row stride 65, the values of the other half going to the spare column.
constexpr int OFF32_UNPERM_LD = 65;
static_assert(4 * 32 * OFF32_UNPERM_LD <= OFF32_STAGE_FLOATS, "the four waves' un-permute buffers fit in the staging buffers");

template <int HB, bool SC = false>   // HB 0: dense H; HB_MODE_SCATTER / HB_MODE_ROUNDS: block-compact H, how a tile's pieces reach the accumulators
__global__ void __launch_bounds__(256, 2)
chol_offdiag_f32_kernel(const float* __restrict__ H, float* __restrict__ L, const float* __restrict__ panel, int n,
                        int64_t ld, int jarg, int ntiles, int i_first, int nrow_tiles, int B, TilePat pat, HBlk hb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  // Default map: the problem is the slow index -- all row tiles of a problem run at the same time on ONE XCD and share the column
  // panel in its L2.  pat.lpt (small-batch tile-sparse launches, the look-ahead schedule): the ENTRY is the slow index, i.e. the
  // column's entries are dispatched longest K-list first (a band's entries are sorted that way: the nearer the diagonal, the
  // longer) -- with two to three rounds of workgroups per launch the tail of a LONG tile started last costs more than the panel
  // re-reads (same-box A/B profiles/r4/s_: banded BA system 6.62 -> 6.34 / 6.46 ms, bit-identical factor).
  const int b8 = gridDim.x / (8 * nrow_tiles);
  const int b = pat.lpt ? (slot % b8) * 8 + xcd : (slot / nrow_tiles) * 8 + xcd;
  const int rslot = pat.lpt ? slot / b8 : slot % nrow_tiles;
  // row tiles [i_first, i_first + nrow_tiles) of block column j -- or, tile-sparse, entries [i_first, i_first + nrow_tiles) of the
  // column's list of non-zero row tiles
  // (tile-sparse: i_first = first ENTRY of the launch, relative to the column's list -- level schedule: absolute, and the entry
  //  names its block column)
  const int ent = pat.col_row ? (pat.ent_col ? 0 : pat.col_ptr[jarg]) + i_first + rslot : 0;
  // right-looking trailing update of block column jc (pat.rl = 2 + jc; dense frames): slot t -> tile (i, k), jc < k <= i,
  // rows of the lower triangle numbered row by row; "j" is the tile's own block column k, the K-loop is the one tile jc
  const bool combo = pat.rl_nsub > 0;   // (TilePat.rl_nsub: substitution tiles of column jarg + update tiles of column jarg - 1)
  const bool upd = combo ? rslot >= pat.rl_nsub : pat.rl >= 2;
  const int jc = combo ? jarg - 1 : pat.rl - 2;
  const int ub = combo ? jarg + 1 : jc + 1;          // first block row / column of the updated tiles
  const bool sla = pat.rl == 1 && pat.rl_la != 0;    // substitution tile with the previous column's update as a one-tile K-loop
  int ui = 0, uk = 0;
  if (upd) {   // (i_first: the launch's first slot)
    const int us = combo ? rslot - pat.rl_nsub : rslot + i_first;
    ui = (int)((__builtin_sqrtf(8.f * (float)us + 1.f) - 1.f) * 0.5f);
    while ((ui + 1) * (ui + 2) / 2 <= us) ++ui;
    while (ui * (ui + 1) / 2 > us) --ui;
    uk = us - ui * (ui + 1) / 2;
  }
  const int j = upd ? ub + uk : (pat.ent_col ? pat.ent_col[ent] : jarg);
  const int i = upd ? ub + ui : (pat.col_row ? pat.col_row[ent] : i_first + rslot);
  const int32_t* klist = pat.col_row ? pat.tile_k + pat.tile_kptr[ent] : nullptr;
  const int Kspan = pat.rl ? ((upd || sla) ? TILE : 0) : (pat.col_row ? (pat.tile_kptr[ent + 1] - pat.tile_kptr[ent]) * TILE : j * TILE);
  const int kcol0 = upd ? jc * TILE : (sla ? (jarg - 1) * TILE : 0);   // first column of the K-loop inside the row panels
  if (b >= B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const LFrame lf = lframe(pat, ld);
  const int64_t mat = (int64_t)b * ld * ld;            // H (dense frame)
  const int64_t lmat = (int64_t)b * lf.pstride;        // L (dense frame or tile-packed)
  const int64_t ldt = lf.ld;
  float* const Lij = L + lmat + lf.tile(i, j, ntiles + ent);   // the tile this workgroup produces
  const int32_t* ksa = lf.packed ? pat.tile_sa + pat.tile_kptr[ent] : nullptr;
  const int32_t* ksb = lf.packed ? pat.tile_sb + pat.tile_kptr[ent] : nullptr;
  const int col0 = j * TILE, row0 = i * TILE;
  const int validB = tile_rows(pat, n, i);  // (columns of tile j beyond the matrix -- last tile / per-tile padding -- come out as exact zeros)
  float* sA = smem;
  float* sB = smem + 128 * 36;
  float* Pc = smem + OFF32_STAGE_FLOATS;

  // ---- prefetch: panel sub-blocks (s,t), t <= s, then the H tile.  Issued from inside the K-loop's prologue, AFTER the
  //      loads of the first k-chunk: one exposed memory latency per workgroup instead of two (in-kernel stamps: 8.8-11.2 k
  //      cycles from kernel entry to the first MFMA, profiles/r2/a_offdiag_stamps.txt) ----
  // (a "lean" variant without any prefetch -- 40 KB LDS, 168 VGPRs, three workgroups per CU -- measured 1-2 % SLOWER:
  //  the K-loop's 82 % MFMA-busy is not an occupancy problem)
  const int r = 32 * wave + (lane & 31), g = lane >> 5;
  const bool rvalid = r < validB;
  float4 hr[4][4];
  HBPre<float, HB ? HB_NPRE_OFF : 1> hbp;
  auto prologue = [&]() __attribute__((always_inline)) {
    if constexpr (HB) hbp.load(hb, b, i, j, tid);
    if constexpr (!HB) {
      const float* Hrow = H + mat + (int64_t)(row0 + (rvalid ? r : 0)) * ld + col0 + 4 * g;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) hr[cb][q] = *reinterpret_cast<const float4*>(Hrow + 32 * cb + 8 * q);
    }
    if (!upd) {  // panel: global -> LDS (swizzled), one 16-byte piece of each of the ten sub-blocks per thread
      const float* Pn = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
      const int pi = tid >> 3, pc = tid & 7;
      float* dst = Pc + pi * 32 + ((pc ^ ((pi >> 1) & 7)) << 2);
      const float* src = Pn + pi * TILE + 4 * pc;
      static_for<4>([&](auto is) __attribute__((always_inline)) {
        constexpr int sb = decltype(is)::value;
        static_for<sb + 1>([&](auto it) __attribute__((always_inline)) {
          constexpr int tb = decltype(it)::value;
          *reinterpret_cast<uint4*>(dst + (sb * (sb + 1) / 2 + tb) * 1024) =
              *reinterpret_cast<const uint4*>(src + 32 * sb * TILE + 32 * tb);
        });
      });
    }
  };

  Engine<float>::Acc P;
  Engine<float>::zero(P);
  // (two LDS staging buffers with ONE barrier per k-chunk instead of one buffer with two -- panel copy moved behind the
  //  loop to keep 2 workgroups/CU -- measured the same 9.3-9.4 k cycles per chunk: the barriers are not the K-loop's limit)
  const float* Ap = L + lmat + (lf.packed ? 0 : (int64_t)col0 * ld) + kcol0;   // rows of block row j (operand A) / i (operand B)
  const float* Bp = L + lmat + (lf.packed ? 0 : (int64_t)row0 * ld) + kcol0;
  const int validA = upd ? tile_rows(pat, n, j) : TILE;   // (update: tile column k may be the LAST block row)
  if constexpr (SC) {
    static_assert(HB != 0, "sorted head-tile columns come with a block-compact H");
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const int32_t __attribute__((address_space(4))) * cmask_t;
    const int32_t* perm = hb.th_perm32 + jarg * TILE;
    const cmask_t pm = (cmask_t)(uintptr_t)(hb.th_mask32 + (int64_t)jarg * 4 * ntiles);
    const cmask_t pk = (cmask_t)(uintptr_t)hb.th_k0h;
    const int nk = Kspan / 32, k0 = min(pk[jarg], nk);
    const int lrow = tid >> 3, lc = tid & 7;
    unsigned voffA[4], voffB[4];   // pass u: staged row lrow + 32 u -- of operand A sorted slot 32 u + lrow, block u
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      voffA[u] = (unsigned)((perm[lrow + 32 * u] * (int)ld + lc * 4) * 4);
      voffB[u] = (unsigned)(((lrow + 32 * u) * (int)ld + lc * 4) * 4);
    }
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Ap), 0, (int)(TILE * ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bp), 0, (int)((int64_t)validB * ld * 4), 0x00020000);
    uint4 ra[2][4], rb[2][4];   // (a piece of A is loaded and staged under the same mask bit)
    auto gload = [&](uint4 (&xa)[4], uint4 (&xb)[4], int kc, int m) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if ((m >> u) & 1) {
          const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rsA, voffA[u], kc * 128, 0);
          xa[u] = make_uint4(a.x, a.y, a.z, a.w);
        }
        const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rsB, voffB[u], kc * 128, 0);
        xb[u] = make_uint4(d.x, d.y, d.z, d.w);
      }
    };
    // the masks of chunks kc .. kc + 3: the prefetch two chunks ahead branches on m2
    int m0 = k0 < nk ? pm[k0] : 0, m1 = k0 + 1 < nk ? pm[k0 + 1] : 0, m2 = k0 + 2 < nk ? pm[k0 + 2] : 0, m3 = k0 + 3 < nk ? pm[k0 + 3] : 0;
    if (k0 < nk) gload(ra[0], rb[0], k0, m0);
    if (k0 + 1 < nk) gload(ra[1], rb[1], k0 + 1, m1);
    prologue();
    const float* sBw = sB + 32 * wave * 36;
    const int rl = lane & 31;
    auto step = [&](uint4 (&xa)[4], uint4 (&xb)[4], int kc) __attribute__((always_inline)) {
      const int mc = m0;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if ((mc >> u) & 1) *reinterpret_cast<uint4*>(sA + (lrow + 32 * u) * 36 + 4 * lc) = xa[u];
        *reinterpret_cast<uint4*>(sB + (lrow + 32 * u) * 36 + 4 * lc) = xb[u];
      }
      __syncthreads();
      if (kc + 2 < nk) gload(xa, xb, kc + 2, m2);
      m0 = m1, m1 = m2, m2 = m3;
      m3 = kc + 4 < nk ? pm[kc + 4] : 0;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {   // (Engine<float>::chunk, block cb only where it is active)
        const float4 fb = *reinterpret_cast<const float4*>(sBw + rl * 36 + 8 * ks + 4 * g);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          if (!((mc >> cb) & 1)) continue;
          const float4 fa = *reinterpret_cast<const float4*>(sA + (32 * cb + rl) * 36 + 8 * ks + 4 * g);
          P.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, P.v[cb], 0, 0, 0);
          P.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, P.v[cb], 0, 0, 0);
          P.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, P.v[cb], 0, 0, 0);
          P.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, P.v[cb], 0, 0, 0);
        }
      }
    };
    for (int kc = k0; kc < nk; kc += 2) {
      step(ra[0], rb[0], kc);
      if (kc + 1 < nk) step(ra[1], rb[1], kc + 1);
    }
    if (k0 < nk) {   // (workgroup uniform; no chunk ran: P is zero in any order)
      __syncthreads();   // the last chunk has been consumed: the staging buffers are free
      float* ub = smem + wave * 32 * OFF32_UNPERM_LD + rl * OFF32_UNPERM_LD;   // this lane's row of the wave's buffer
      int pcol[4][16];   // natural column of this lane's staged columns 32 cb + 8 q + 4 g + k
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int4 pv = *reinterpret_cast<const int4*>(perm + 32 * cb + 8 * q + 4 * g);
          pcol[cb][4 * q] = pv.x, pcol[cb][4 * q + 1] = pv.y, pcol[cb][4 * q + 2] = pv.z, pcol[cb][4 * q + 3] = pv.w;
        }
      Engine<float>::Acc N;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int c = pcol[cb][i] - 64 * h;
            ub[(c >= 0 && c < 64) ? c : 64] = P.v[cb][i];
          }
        wave_lds_fence();
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) N.v[2 * h + cb][4 * q + k] = ub[32 * cb + 8 * q + 4 * g + k];
        wave_lds_fence();
      }
      P = N;
    }
  } else {
  kloop<float, false>(Ap, validA, Bp, validB, ldt, Kspan, sA, sB, P, tid, nullptr, nullptr, prologue, klist, ksa, ksb, lf.pstride);
  }
  if constexpr (HB) {
    // block-compact H: the tile's pieces are gathered into the (now free) staging buffers, 64 rows at a time, and read back in
    // the accumulator layout -- a few hundred elements instead of a 64 KB tile of zeros from HBM
    constexpr int LDH = 132;
    static_assert(64 * LDH <= OFF32_STAGE_FLOATS, "half an H tile must fit in the staging buffers");
    __syncthreads();   // the K-loop's last chunk has been consumed
    // P = -sum first, H_ij's pieces are ADDED
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 16; ++q) P.v[cb][q] = -P.v[cb][q];
    if constexpr (HB == HB_MODE_SCATTER) {
      // a few pieces per tile (pose graphs): added by the matrix cores, see hb_scatter.  (hb_add's barrier also publishes the
      // panel copy -- also when the K-loop had no iterations)
      hb_add<float, Engine<float>::Acc, decltype(hbp), 256 * HB_NPRE_OFF>(P, hbp, hb, b, smem, 0, hbp.cnt / (hb.bd * hb.bd), true, tid);
    } else {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      for (int k = tid; k < 64 * LDH / 4; k += 256) reinterpret_cast<float4*>(smem)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      __syncthreads();
      hbp.foreach(hb, b, tid, [&](int rr, int cc, float v) __attribute__((always_inline)) {
        if ((rr >> 6) == half) smem[(rr & 63) * LDH + cc] = v;
      });
      __syncthreads();
      if ((wave >> 1) == half) {
        const float* hrow = smem + (r & 63) * LDH + 4 * g;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 h = *reinterpret_cast<const float4*>(hrow + 32 * cb + 8 * q);
            P.v[cb][4 * q + 0] = h.x + P.v[cb][4 * q + 0];   // (P holds -sum already)
            P.v[cb][4 * q + 1] = h.y + P.v[cb][4 * q + 1];
            P.v[cb][4 * q + 2] = h.z + P.v[cb][4 * q + 2];
            P.v[cb][4 * q + 3] = h.w + P.v[cb][4 * q + 3];
          }
      }
      __syncthreads();
    }
    }
  } else {
    // P = H_ij - sum (rows outside the matrix: zero)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 h = hr[cb][q];
        P.v[cb][4 * q + 0] = (rvalid ? h.x : 0.f) - P.v[cb][4 * q + 0];
        P.v[cb][4 * q + 1] = (rvalid ? h.y : 0.f) - P.v[cb][4 * q + 1];
        P.v[cb][4 * q + 2] = (rvalid ? h.z : 0.f) - P.v[cb][4 * q + 2];
        P.v[cb][4 * q + 3] = (rvalid ? h.w : 0.f) - P.v[cb][4 * q + 3];
      }
    __syncthreads();  // panel copy visible (also when the K-loop had no iterations)
  }
  if (upd) {   // trailing update: the tile goes back as it is (a diagonal tile: its lower triangle, zeros above)
    if (rvalid) {
      float* Lrow = Lij + (int64_t)r * ldt + 4 * g;
      const int rt = 32 * wave + (lane & 31);   // row inside the tile
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = 32 * cb + 8 * q + 4 * g;
          const bool dg = i == j;
          *reinterpret_cast<float4*>(Lrow + 32 * cb + 8 * q) =
              make_float4(dg && c + 0 > rt ? 0.f : P.v[cb][4 * q], dg && c + 1 > rt ? 0.f : P.v[cb][4 * q + 1],
                          dg && c + 2 > rt ? 0.f : P.v[cb][4 * q + 2], dg && c + 3 > rt ? 0.f : P.v[cb][4 * q + 3]);
        }
    }
    return;
  }
  Engine<float>::Acc X;
  Engine<float>::zero(X);
  static_for<4>([&](auto is) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value;
    static_for<sb>([&](auto it) __attribute__((always_inline)) {
      constexpr int tb = decltype(it)::value;
      sub_mma_sw<sb, tb>(Pc, X, P, lane);  // P_s += (-L_st) X_t
    });
    sub_mma_sw<sb, sb>(Pc, P, X, lane);    // X_s  = W_ss P_s
  });
  if (rvalid) {
    float* Lrow = Lij + (int64_t)r * ldt + 4 * g;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(Lrow + 32 * cb + 8 * q) =
            make_float4(X.v[cb][4 * q], X.v[cb][4 * q + 1], X.v[cb][4 * q + 2], X.v[cb][4 * q + 3]);
  }
  if (pat.rl_y) {   // right-looking forward substitution: block i of the vector loses L_ij y_j (a row's 128 columns sit in two lanes)
    float* yb = static_cast<float*>(pat.rl_y) + (int64_t)b * pat.rl_ldv;
    const float* yj = yb + col0 + 4 * g;
    float dot = 0.f;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 yv = *reinterpret_cast<const float4*>(yj + 32 * cb + 8 * q);
        dot += X.v[cb][4 * q] * yv.x + X.v[cb][4 * q + 1] * yv.y + X.v[cb][4 * q + 2] * yv.z + X.v[cb][4 * q + 3] * yv.w;
      }
    dot += __shfl_xor(dot, 32);
    if (g == 0 && rvalid) yb[row0 + r] -= dot;
  }
}

// ------------------------------------------------------------------------------------------------
// chol_offdiag2, fp32, dense L frame: tiles (i, j) AND (i, j + 1) of row tile i >= j + 2 in one workgroup (round 5).
// Under thx_chol_factor the socket sits at its 1400 W cap (rocm-smi: 1356 W, 2.2 GHz; an HBM copy alone costs ~140 W per
// TB/s, profiles/r5/q_, r_): the factorisation's 2.7 TB/s are a quarter of its power.  Left-looking, tile (i, j) streams row
// panel L_i,0:j once per COLUMN j; here it is streamed once per column PAIR -- the K-loop over block columns 0 .. j - 1 stages
// three operand chunks (rows j, rows j + 1, rows i) for two tile products (4 for 2 before: -25 % operand loads, staging stores
// and barriers per MFMA, half the row-panel bytes from HBM), then
//   X0 = (H_ij - P0) L_jj^-T                      (the substitution of chol_offdiag, stored as L_ij)
//   P1 += X0 L_{j+1,j}^T                           (block column j's share of tile (i, j + 1): X0 stays in the accumulator
//                                                   registers and is the MFMAs' B operand itself -- an MFMA's k index is only a
//                                                   pairing of columns, and the accumulator layout pairs its columns the way the
//                                                   staged fragments do; the four chunks of L_{j+1,j} are staged as in the K-loop)
//   X1 = (H_i,j+1 - P1) L_{j+1,j+1}^-T
// Every accumulator receives the SAME MFMAs in the SAME order as in chol_offdiag_f32_kernel: the factor is bit-identical.
// Needs diag(j), tile (j + 1, j) and diag(j + 1) before it: the host launches column j's head tile alone (factor_impl).
// LDS 76 KB (two workgroups per CU): [0, 54 KB) three staging buffers | [36 KB, 76 KB) the panel copy of the substitution in
// progress (lands there straight from global memory after the K-loop; overlaps the third staging buffer only).
// RG (FactorPlan.regroup, HBlk.rg_*): the workgroup's 128 rows are a ROW GROUP instead of row tile i -- the rows below the pair
// sorted by their first non-zero column, so that the K-loop starts at the group's first non-zero chunk k0 (every row of the
// group is zero left of it: exact zeros left out, as with the sub-block masks, but for the whole workgroup -- no loads, staging
// stores or barriers for those chunks).  Every row of L is independent here and keeps its own products in their order: L is
// bit-identical (up to the sign of a zero).  The group's rows come from a table (operand B's row offsets, the rows stored to),
// its pieces of H from tables keyed by (group, block column); the row-side sub-block mask has no meaning for a group and is gone.
// ZERO SOLVES (FactorPlan.zsolve, HBlk.rg_zf): each wave's 32 rows have a first non-zero chunk of their own, not capped at 4 j.  The
// wave leaves out the k-chunks in front of it and, where its rows begin inside or behind the pair's columns, the sub-blocks of the
// two substitutions and the coupling products whose operand is zero; a group that lies wholly behind block column j (or the
// pair) stores zeros for that tile (both tiles) and skips the tile's loads, staging and barriers as a workgroup.  Pair 0 -- no
// K-loop, so no groups of the kind above -- runs on groups of its own through the same instantiation (pair_groups0).  The same
// products in the same order for every element that is computed; what is left out is a product with an exact zero.
// ------------------------------------------------------------------------------------------------
constexpr int OFF2_PANEL_OFF = 2 * 128 * 36;              // floats: right behind staging buffers 0 and 1
constexpr int OFF2_SMEM = (OFF2_PANEL_OFF + 10 * 1024) * 4;   // 76 KB
static_assert(64 * 132 <= OFF2_PANEL_OFF, "the H gather (half a tile) must not touch the panel copy");
static_assert(2 * 128 * 36 <= OFF2_PANEL_OFF, "staging buffers 0 and 1 must not touch the panel copy");
static_assert(OFF2_SMEM >= 3 * 128 * 36 * 4 && 2 * OFF2_SMEM <= 160 * 1024, "three staging buffers; two workgroups per CU");

// SORTED COLUMNS (SC; FactorPlan.sortcols, HBlk.sc_perm / sc_mask of THIS pair): the column side of the K-loop gets what the row
// groups gave the row side.  The pair's 256 columns c -- the rows of tiles j, j + 1, operand A -- are staged in ascending order of
// their first non-zero column: staged block u of sA0 / sA1 (32 rows) holds sorted slots 32 u .. / 128 + 32 u ..., and is all zero at
// a chunk as long as its FIRST row has not begun.  sc_mask[kc] names the eight blocks' active ones: for the others the loads, the
// staging stores and the MFMAs are left out (workgroup-uniform, as the m0 / m1 branch).  Every column accumulates independently
// of the others and keeps its products in their order; P0 / P1 hold sorted slots until the K-loop ends and are then moved to natural
// column order through LDS, 128 columns at a time, each wave its own 32 rows.  Everything behind runs on natural P0 / P1.
constexpr int OFF2_UNPERM_LD = 129;   // row stride of the un-permute buffer: 128 columns + one that takes the other half's values
static_assert(4 * 32 * OFF2_UNPERM_LD * 4 <= OFF2_SMEM, "the four waves' un-permute buffers fit in the kernel's LDS");

template <int HB, bool RG = false, bool SC = false>   // (HB as chol_offdiag_f32_kernel; RG: i_first is the pair's first GROUP, nrow_tiles its group count)
__global__ void __launch_bounds__(256, 2)
chol_offdiag2_f32_kernel(const float* __restrict__ H, float* __restrict__ L, const float* __restrict__ panel, int n,
                         int64_t ld, int j, int ntiles, int i_first, int nrow_tiles, int B, HBlk hb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* smem = reinterpret_cast<float*>(smem_raw);
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int b = (slot / nrow_tiles) * 8 + xcd;   // problem-major: all row tiles of a problem on ONE XCD (panel rows j, j + 1 in its L2)
  const int i = i_first + slot % nrow_tiles;     // (RG: the group)
  if (b >= B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t mat = (int64_t)b * ld * ld;
  const int col0 = j * TILE, row0 = i * TILE;
  const int validB = min(TILE, n - row0);
  static_assert(!RG || HB != 0, "row groups come with a block-compact H");
  HBlk hq = hb;   // where the workgroup's pieces of H are listed
  if constexpr (RG) {
    hq.tile_ptr = hb.rg_tile_ptr;
    hq.piece_blk = hb.rg_piece_blk;
    hq.piece_rc = hb.rg_piece_rc;
  }
  float* sA0 = smem;
  float* sA1 = smem + 128 * 36;
  float* sB = smem + 2 * 128 * 36;
  float* Pc = smem + OFF2_PANEL_OFF;
  const int r = 32 * wave + (lane & 31), g = lane >> 5, rl = lane & 31;
  int srow = row0 + r;   // the matrix row of this lane's row of the workgroup
  if constexpr (RG) srow = hb.rg_rows[i * TILE + r];
  const bool rvalid = RG ? srow >= 0 : r < validB;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef const int32_t __attribute__((address_space(4))) * lmask_t;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int nk = 4 * j;
  // ZERO SOLVES (HBlk.rg_zf, nullptr: none -- everything below is then 0): this wave's 32 rows are zero left of chunk zf.  z of the pair's
  // eight 32-column sub-blocks are zero for the wave, z0 of them in tile (i, j), z1 in tile (i, j + 1); zall: the same for the
  // wave of the group that begins first.  All of it in scalar registers: every branch on them is wave or workgroup uniform.
  int zf = 0, zmin = 0;
  if constexpr (RG) {
    const lmask_t zt = (lmask_t)(uintptr_t)hb.rg_zf;
    if (zt) {
      zf = zt[4 * i + wv];
      zmin = min(min(zt[4 * i], zt[4 * i + 1]), min(zt[4 * i + 2], zt[4 * i + 3]));
    }
  }
  const int z = min(max(zf - nk, 0), 8), z0 = RG ? min(z, 4) : 0, z1 = RG ? z - z0 : 0;
  const int zall = RG ? min(max(zmin - nk, 0), 8) : 0;
  // rows of the group that are zero in ncb 32-column sub-blocks from column col0 on: the zeros are STORED (L may hold anything,
  // and the SYRK / head-tile kernels and the solves read whole rows)
  auto store_zeros = [&](int ncb) __attribute__((always_inline)) {
    if (rvalid) {
      float* Lrow = L + mat + (int64_t)srow * ld + col0 + 4 * g;
      for (int cb = 0; cb < ncb; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<float4*>(Lrow + 32 * cb + 8 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  if constexpr (RG)
    if (zall == 8) {   // every row of the group begins behind the pair: both tiles are zeros, nothing to load
      store_zeros(8);
      return;
    }

  HBPre2<float, HB ? 2 * HB_NPRE_OFF : 1> hb2;
  // ---- K-loop over block columns 0 .. j - 1: P0 += L_i L_j^T, P1 += L_i L_{j+1}^T ----
  static_assert(!SC || RG, "sorted columns come with row groups");
  const int lrow = tid >> 3, lc = tid & 7;
  unsigned voff[4];
  auto natural_voff = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) voff[u] = (unsigned)(((lrow + 32 * u) * (int)ld + lc * 4) * 4);
  };
  if constexpr (!SC) natural_voff();   // (SC: the K-loop has offsets of its own, these are made behind it for gload1)
  // SC: operand A's staged row lrow + 32 u of sA0 / sA1 is the pair's sorted slot 32 u + lrow / 128 + 32 u + lrow -- row sc_perm[slot]
  // of the 256 rows from col0 on
  unsigned voffA0[4], voffA1[4];
  if constexpr (SC) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      voffA0[u] = (unsigned)((hb.sc_perm[lrow + 32 * u] * (int)ld + lc * 4) * 4);
      voffA1[u] = (unsigned)((hb.sc_perm[128 + lrow + 32 * u] * (int)ld + lc * 4) * 4);
    }
  }
  // operand B's rows: RG -- the group's rows anywhere in the frame (the host checked n * ld * 4 < 2^31); a slot without a row is
  // out of the buffer's range and reads zeros, as the rows behind the matrix do
  unsigned voffB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    voffB[u] = voff[u];
    if constexpr (RG) {
      const int rw = hb.rg_rows[i * TILE + lrow + 32 * u];
      voffB[u] = rw < 0 ? 0x80000000u : (unsigned)((rw * (int)ld + lc * 4) * 4);
    }
  }
  const float* Lb = L + mat;
  const __amdgpu_buffer_rsrc_t rsA0 =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lb + (int64_t)col0 * ld), 0, (int)(TILE * ld * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA1 =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lb + (int64_t)(col0 + TILE) * ld), 0, (int)(TILE * ld * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lb + (RG ? (int64_t)0 : (int64_t)row0 * ld)), 0,
                                        (int)((RG ? n : validB) * ld * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsA =   // (SC: the rows of both tiles, sorted slots point anywhere in them)
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Lb + (int64_t)col0 * ld), 0, (int)(2 * TILE * ld * 4), 0x00020000);
  uint4 q0[4], q1[4], qb[4];
  // (SC: am, the chunk's 8-bit mask of active sorted blocks -- block u of sA0 is bit u, of sA1 bit 4 + u; an inactive block is not loaded)
  auto gload3 = [&](int kc, int am) __attribute__((always_inline)) {
    const int so = kc * 32 * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (SC) {
        if ((am >> u) & 1) {
          const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rsA, voffA0[u], so, 0);
          q0[u] = make_uint4(a.x, a.y, a.z, a.w);
        }
        if ((am >> (4 + u)) & 1) {
          const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(rsA, voffA1[u], so, 0);
          q1[u] = make_uint4(c.x, c.y, c.z, c.w);
        }
      } else {
        const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rsA0, voff[u], so, 0);
        const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(rsA1, voff[u], so, 0);
        q0[u] = make_uint4(a.x, a.y, a.z, a.w);
        q1[u] = make_uint4(c.x, c.y, c.z, c.w);
      }
      const u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rsB, voffB[u], so, 0);
      qb[u] = make_uint4(d.x, d.y, d.z, d.w);
    }
  };
  auto gload1 = [&](int kc) __attribute__((always_inline)) {   // rows j + 1 only (block column j's share)
    const int so = kc * 32 * 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(rsA1, voff[u], so, 0);
      q1[u] = make_uint4(c.x, c.y, c.z, c.w);
    }
  };
  Engine<float>::Acc P0, P1;
  Engine<float>::zero(P0);
  Engine<float>::zero(P1);
  int k0 = 0;   // first chunk of the K-loop
  if constexpr (RG)   // (with the strips' table min(zmin, nk) is rg_k0[i], min(min first / 32, 4 j); pair 0's tables have no rg_k0)
    k0 = hb.rg_zf ? min(zmin, nk) : __builtin_amdgcn_readfirstlane(hb.rg_k0[i]);
  // SC: the masks come two chunks ahead of the MFMAs -- the next chunk's loads branch on theirs (scm1), and a scalar load issued with
  // those loads (scm2) has completed under a whole chunk's MFMAs by the time it is needed
  const lmask_t scm = (lmask_t)(uintptr_t)hb.sc_mask;
  int scm1 = 255, scm2 = 255;
  if constexpr (SC) {
#pragma unroll
    for (int u = 0; u < 4; ++u) q0[u] = q1[u] = make_uint4(0u, 0u, 0u, 0u);
    if (nk > k0) scm1 = scm[k0];
    if (nk > k0 + 1) scm2 = scm[k0 + 1];
  }
  if (nk > k0) gload3(k0, scm1);
  if constexpr (RG) hb2.load_run(hq, b, 2 * i, tid);
  else if constexpr (HB) hb2.load(hb, b, i, j, tid);
  const float* sBw = sB + 32 * wave * 36;
  // Structurally zero 32x32 sub-blocks of L (HBlk.l_mask, nullptr: none): per k-chunk the 4-bit masks of tiles j, j + 1 (the
  // column side: operand A sub-block cb, the same for the four waves) and of row tile i (the row side: this wave's operand B
  // sub-block).  An MFMA of an all-zero operand adds exact zeros: its output block's products are left out (wave-uniform
  // branches), every accumulator still receives the others in the same order.  Scalar loads through the constant address space
  // (as kloop_f's K-list), one chunk ahead: issued with the chunk's operand prefetch, they complete under the MFMAs.
  const lmask_t lm = (lmask_t)(uintptr_t)(SC ? nullptr : hb.l_mask);   // (SC: the natural-order masks say nothing about sorted blocks)
  const int nch = 4 * ntiles;
  int nm0 = 15, nm1 = 15, nmi = 15;   // the masks of the next chunk
  auto lmask_load = [&](int kc) __attribute__((always_inline)) {
    if (lm) {
      nm0 = lm[j * nch + kc];
      nm1 = lm[(j + 1) * nch + kc];
      if constexpr (!RG) nmi = lm[i * nch + kc];
    }
  };
  if (nk > k0) lmask_load(k0);
  for (int kc = k0; kc < nk; ++kc) {
    const int m0 = SC ? (scm1 & 15) : nm0, m1 = SC ? (scm1 >> 4) : nm1, mi = nmi;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = lrow + 32 * u;
      if (!SC || ((m0 >> u) & 1)) *reinterpret_cast<uint4*>(sA0 + row * 36 + 4 * lc) = q0[u];
      if (!SC || ((m1 >> u) & 1)) *reinterpret_cast<uint4*>(sA1 + row * 36 + 4 * lc) = q1[u];
      *reinterpret_cast<uint4*>(sB + row * 36 + 4 * lc) = qb[u];
    }
    __syncthreads();
    if constexpr (SC) {
      scm1 = scm2;
      if (kc + 1 < nk) gload3(kc + 1, scm1);
      if (kc + 2 < nk) scm2 = scm[kc + 2];
    } else if (kc + 1 < nk) {
      gload3(kc + 1, 255);
      lmask_load(kc + 1);
    }
    if constexpr (!RG)
      if (!((mi >> wv) & 1)) continue;   // this wave's rows of L_i are zero at the chunk: nothing to add
    if constexpr (RG)
      if (kc < zf) continue;             // ... the same, from the strip's first chunk
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 fb = *reinterpret_cast<const float4*>(sBw + rl * 36 + 8 * ks + 4 * g);
      float4 fa0[4], fa1[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        fa0[cb] = *reinterpret_cast<const float4*>(sA0 + (32 * cb + rl) * 36 + 8 * ks + 4 * g);
        fa1[cb] = *reinterpret_cast<const float4*>(sA1 + (32 * cb + rl) * 36 + 8 * ks + 4 * g);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        if (!((m0 >> cb) & 1)) continue;
        const float4 fa = fa0[cb];
        P0.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, P0.v[cb], 0, 0, 0);
        P0.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, P0.v[cb], 0, 0, 0);
        P0.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, P0.v[cb], 0, 0, 0);
        P0.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, P0.v[cb], 0, 0, 0);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        if (!((m1 >> cb) & 1)) continue;
        const float4 fa = fa1[cb];
        P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, P1.v[cb], 0, 0, 0);
        P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, P1.v[cb], 0, 0, 0);
        P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, P1.v[cb], 0, 0, 0);
        P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, P1.v[cb], 0, 0, 0);
      }
    }
  }

  // panel of diagonal tile jj: global -> LDS directly (global_load_lds: no registers -- ten pieces per thread held across the H
  // gather were spilled), in the substitution's swizzled layout: LDS slot (row pi, 16-byte slot ps) of a sub-block receives the
  // row's piece ps ^ ((pi >> 1) & 7); a wave fills 1 KB of consecutive slots per instruction
  auto panel_dma = [&](int jj) __attribute__((always_inline)) {
    const float* Pn = panel + ((int64_t)b * ntiles + jj) * TILE * TILE;
    const int pi = 8 * wave + (lane >> 3), pc = (lane & 7) ^ ((pi >> 1) & 7);
    const float* src = Pn + pi * TILE + 4 * pc;
    static_for<4>([&](auto is) __attribute__((always_inline)) {
      constexpr int sb = decltype(is)::value;
      static_for<sb + 1>([&](auto it) __attribute__((always_inline)) {
        constexpr int tb = decltype(it)::value;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 32 * sb * TILE + 32 * tb),
                                         (__attribute__((address_space(3))) void*)(Pc + (sb * (sb + 1) / 2 + tb) * 1024 + wave * 256),
                                         16, 0, 0);
      });
    });
  };
  // P <- H_(i, jj) - P  (block-compact H: the tile's pieces through the free staging buffers, 64 rows at a time; dense: loads)
  auto h_minus = [&](Engine<float>::Acc& P, int sel, int jj, bool first) __attribute__((always_inline)) {   // (first: no call before it)
    if constexpr (HB) {
      constexpr int LDH = 132;
      // P = -sum first, H's pieces are ADDED
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 16; ++q) P.v[cb][q] = -P.v[cb][q];
      if constexpr (HB == HB_MODE_SCATTER) {
        // a few pieces per tile (pose graphs): added by the matrix cores, see hb_scatter.  Both tiles' values go to staging
        // buffer 0 as ONE list before tile (i, j)'s pieces are applied (the caller's barrier before panel_dma(j): the K-loop is
        // done with the buffers); nothing writes that buffer until tile (i, j + 1)'s turn (column j's share of it is staged in
        // buffer 1): no second copy, no second barrier.  (Tile (i, j) left out: tile (i, j + 1)'s call is the first and stages the list.)
        const int n0 = hb2.p1 - hb2.p0, ntot = hb2.cnt / (hb.bd * hb.bd);
        static_assert(256 * 2 * HB_NPRE_OFF + 64 * 36 <= 128 * 36, "list + overflow chunk inside staging buffer 0");
        hb_add<float, Engine<float>::Acc, decltype(hb2), 256 * 2 * HB_NPRE_OFF>(P, hb2, hq, b, smem, sel == 0 ? 0 : n0, sel == 0 ? n0 : ntot,
                                                                               first, tid);
      } else {
      __syncthreads();   // whatever read the staging buffers last is done
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        for (int k = tid; k < 64 * LDH / 4; k += 256) reinterpret_cast<float4*>(smem)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        hb2.foreach(hq, b, tid, sel, [&](int rr, int cc, float v) __attribute__((always_inline)) {
          if ((rr >> 6) == half) smem[(rr & 63) * LDH + cc] = v;
        });
        __syncthreads();
        if ((wave >> 1) == half) {
          const float* hrow = smem + (r & 63) * LDH + 4 * g;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float4 h = *reinterpret_cast<const float4*>(hrow + 32 * cb + 8 * q);
              P.v[cb][4 * q + 0] = h.x + P.v[cb][4 * q + 0];   // (P holds -sum already)
              P.v[cb][4 * q + 1] = h.y + P.v[cb][4 * q + 1];
              P.v[cb][4 * q + 2] = h.z + P.v[cb][4 * q + 2];
              P.v[cb][4 * q + 3] = h.w + P.v[cb][4 * q + 3];
            }
        }
        __syncthreads();
      }
      }
    } else {
      const float* Hrow = H + mat + (int64_t)(row0 + (rvalid ? r : 0)) * ld + jj * TILE + 4 * g;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        float4 h[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) h[q] = *reinterpret_cast<const float4*>(Hrow + 32 * cb + 8 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          P.v[cb][4 * q + 0] = (rvalid ? h[q].x : 0.f) - P.v[cb][4 * q + 0];
          P.v[cb][4 * q + 1] = (rvalid ? h[q].y : 0.f) - P.v[cb][4 * q + 1];
          P.v[cb][4 * q + 2] = (rvalid ? h[q].z : 0.f) - P.v[cb][4 * q + 2];
          P.v[cb][4 * q + 3] = (rvalid ? h[q].w : 0.f) - P.v[cb][4 * q + 3];
        }
      }
    }
  };
  // X = P L_jj^-T with the panel copy in LDS (chol_offdiag's substitution), X -> tile (i, jj) of L.  zs: the wave's first zs
  // sub-blocks of P are structurally zero -- X_t = 0 for t < zs, left as zeroed, and its products with them are left out
  auto substitute_store = [&](Engine<float>::Acc& P, Engine<float>::Acc& X, int jj, int zs) __attribute__((always_inline)) {
    Engine<float>::zero(X);
    static_for<4>([&](auto is) __attribute__((always_inline)) {
      constexpr int sb = decltype(is)::value;
      if (sb >= zs) {
        static_for<sb>([&](auto it) __attribute__((always_inline)) {
          constexpr int tb = decltype(it)::value;
          if (tb >= zs) sub_mma_sw<sb, tb>(Pc, X, P, lane);  // P_s += (-L_st) X_t
        });
        sub_mma_sw<sb, sb>(Pc, P, X, lane);    // X_s  = W_ss P_s
      }
    });
    if (rvalid) {
      float* Lrow = L + mat + (int64_t)srow * ld + jj * TILE + 4 * g;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<float4*>(Lrow + 32 * cb + 8 * q) =
              make_float4(X.v[cb][4 * q], X.v[cb][4 * q + 1], X.v[cb][4 * q + 2], X.v[cb][4 * q + 3]);
    }
  };

  if constexpr (SC) {
    natural_voff();
    // ---- un-permute: P0 / P1 hold the pair's columns in sorted order, lane (rl, g) those of row 32 wave + rl at sorted slots
    //      32 cb + 8 q + 4 g + s.  Two rounds of 128 natural columns (tile j -> P0, tile j + 1 -> P1): the lane writes all of its 256
    //      values to row rl of the wave's buffer, a value of the other tile to the row's spare column 128, and reads its natural
    //      columns back.  Round 0's values wait in T until round 1 has read P0 / P1 for the last time.  A wave's LDS operations
    //      execute in order and only its own lanes touch its buffer; the barrier in front separates them from the K-loop's last
    //      chunk, the one behind (tile (i, j)'s, below) from the panel copy, which lands on top of these buffers.
    if (nk > k0) {   // (else P0 = P1 = 0; zall < 4 then: the branch below opens with the barrier behind)
      __syncthreads();
      if (zf < nk) {   // (else this wave ran no chunk)
        float* ub = smem + wave * (32 * OFF2_UNPERM_LD) + rl * OFF2_UNPERM_LD;
        Engine<float>::Acc T;
        auto round = [&](int t, Engine<float>::Acc& D) __attribute__((always_inline)) {
#pragma unroll
          for (int cb = 0; cb < 8; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int4 pv = *reinterpret_cast<const int4*>(hb.sc_perm + 32 * cb + 8 * q + 4 * g);
              const Engine<float>::Acc& S = cb < 4 ? P0 : P1;
              ub[min((unsigned)(pv.x - 128 * t), 128u)] = S.v[cb & 3][4 * q + 0];
              ub[min((unsigned)(pv.y - 128 * t), 128u)] = S.v[cb & 3][4 * q + 1];
              ub[min((unsigned)(pv.z - 128 * t), 128u)] = S.v[cb & 3][4 * q + 2];
              ub[min((unsigned)(pv.w - 128 * t), 128u)] = S.v[cb & 3][4 * q + 3];
            }
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 16; ++q) D.v[cb][q] = ub[32 * cb + 8 * (q >> 2) + 4 * g + (q & 3)];
          __builtin_amdgcn_wave_barrier();
        };
        round(0, T);
        round(1, P1);
        P0 = T;
      }
    }
  }

  Engine<float>::Acc X0;
  bool first = true;   // (no h_minus call yet)
  if (!RG || zall < 4) {
    // ---- tile (i, j) ----
    __syncthreads();      // the K-loop's last chunk has been consumed: the panel copy overlaps staging buffer 2
    panel_dma(j);
    h_minus(P0, 0, j, true);
    first = false;
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the panel have landed
    __syncthreads();
    gload1(nk);           // first chunk of L_{j+1,j}: in flight under the substitution
    substitute_store(P0, X0, j, z0);
    // ---- block column j's share of tile (i, j + 1): P1 += X0 L_{j+1,j}^T, X0 from registers (chunk c of X0 zero: only the
    //      wave's MFMAs are left out, the chunk is staged for the others) ----
    static_for<4>([&](auto ic) __attribute__((always_inline)) {
      constexpr int c = decltype(ic)::value;
      __syncthreads();    // (c = 0: the substitution's reads of the panel copy are done as well)
#pragma unroll
      for (int u = 0; u < 4; ++u) *reinterpret_cast<uint4*>(sA1 + (lrow + 32 * u) * 36 + 4 * lc) = q1[u];
      __syncthreads();
      if (c == 0) panel_dma(j + 1);   // lands under the four chunks' MFMAs
      if (c < 3) gload1(nk + c + 1);
      if (c >= z0) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) {
            const float4 fa = *reinterpret_cast<const float4*>(sA1 + (32 * cb + rl) * 36 + 8 * ks + 4 * g);
            P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, X0.v[c][4 * ks + 0], P1.v[cb], 0, 0, 0);
            P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, X0.v[c][4 * ks + 1], P1.v[cb], 0, 0, 0);
            P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, X0.v[c][4 * ks + 2], P1.v[cb], 0, 0, 0);
            P1.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, X0.v[c][4 * ks + 3], P1.v[cb], 0, 0, 0);
          }
        }
      }
    });
  } else {
    // every row of the group begins behind block column j: tile (i, j) is zeros and adds nothing to tile (i, j + 1).  The K-loop
    // had no iterations (k0 = 4 j): LDS is untouched so far
    store_zeros(4);
    panel_dma(j + 1);
  }
  // ---- tile (i, j + 1) ----
  h_minus(P1, 1, j + 1, first);
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
  __syncthreads();
  substitute_store(P1, X0, j + 1, z1);
}

// (A variant computing TWO row tiles per workgroup -- the column panel streamed once for both products, 3 staged operand
//  tiles per 2 tile products, half the workgroups, H / panel loaded after the K-loop, 240 VGPRs, 54 KB LDS -- measured
//  48.5 ms against 48.3 ms for this kernel on the same box at n = 1536, batch 4096, and the same at n = 3072 / batch 256 and
//  batch 1024: what it saves per tile in the prologue and the K-loop it gives back in the exposed loads and the longer
//  substitution phase.  Not kept; profiles/r2/f_pair_kernel_ab.txt.)

}  // namespace thx
