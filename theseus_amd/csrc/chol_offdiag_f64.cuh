#pragma once
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_engine.cuh"
#include "chol_tiles.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// chol_offdiag, fp64: two workgroups per CU (a full 128x130 fp64 panel tile in LDS would be 133 KB):
//   * H_ij and the result go global <-> registers directly in the accumulator's native layout (a 4-lane group covers 32
//     contiguous bytes of a row);
//   * the panel's lower 32x32 sub-blocks are staged compactly (8 KB each, XOR-swizzled: conflict-free ds_read_b64 of the
//     A fragments) in two phases -- rows 0..2 (48 KB), then row 3 -- over the K-loop's staging buffers;
//   * the substitution runs IN PLACE: X_s = W_ss P_s goes through a 32-VGPR temporary back into P_s's registers, which
//     then serve as the B operand of the updates P_u += (-L_us) X_s.  128 + 32 accumulator VGPRs instead of 256.
// ------------------------------------------------------------------------------------------------
// LDS of the fp64 off-diagonal kernel (round 4): the K-loop's staging buffers (2 x 128 x LDT doubles = 36.9 KB with 16-column
// chunks; after the K-loop: four 8 KB panel sub-blocks) + a 40 KB region E for panel sub-blocks 0..4, which land there straight
// from global memory (global_load_lds, no registers) while the FIRST k-chunk is in flight -- 76.9 KB, two workgroups per CU.
// The substitution starts on E the moment the K-loop ends; sub-blocks 5..8 are requested then (LDS-direct into the staging buffers)
// and arrive under its first five block products, W_33 takes sub-block 0's place in E under the next four.  (Round 3: all ten
// sub-blocks were fetched after the K-loop, in two phases, each an exposed round trip.)
constexpr int OFF64_STAGE = (2 * 128 * CT<double>::LDT * 8 > 4 * 1024 * 8) ? 2 * 128 * CT<double>::LDT * 8 : 4 * 1024 * 8;
constexpr int OFF64_EBLK = 5;
constexpr int OFF64_SMEM = OFF64_STAGE + OFF64_EBLK * 1024 * 8;
static_assert(2 * OFF64_SMEM <= 160 * 1024, "two fp64 off-diagonal workgroups per CU");

// D.block(S) += Pc[block idx] * Bs.block(Tt)^T, Pc block: 32 x 32 doubles, element (r, c) at r * 32 + (c ^ 2 (r & 15))
template <int S, int Tt, typename DT>
__device__ __forceinline__ void sub_mma64(const double* blk, const Engine<double>::Acc& Bs, DT& D0, DT& D1, int lane) {
  // D0 / D1: the two 16-column accumulator blocks [h] of sub-block S: f64x4 (&)[2] each ([h])
  const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {       // 16-row half of the panel sub-block <-> accumulator block cp = 2S + ch
#pragma unroll
    for (int cbh = 0; cbh < 2; ++cbh)    // 16-column half <-> B block cb = 2Tt + cbh
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const int r = 16 * ch + rl, c = 16 * cbh + 4 * rho + kq;
        const double a = blk[r * 32 + (c ^ (2 * rl))];
        auto& d = ch == 0 ? D0 : D1;
        d[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs.v[0][2 * Tt + cbh][rho], d[0], 0, 0, 0);
        d[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs.v[1][2 * Tt + cbh][rho], d[1], 0, 0, 0);
      }
  }
}

template <int HB, bool RL = false>    // (HB: as chol_offdiag_f32_kernel; RL: the right-looking schedule's modes, TilePat.rl / rl_y -- an instance of its own: in the
                                      //  left-looking instance the extra live values spilled 268 - 700 B per lane through scratch)
__global__ void __launch_bounds__(256, 2)
chol_offdiag_f64_kernel(const double* __restrict__ H, double* __restrict__ L, const double* __restrict__ panel, int n,
                        int64_t ld, int jarg, int ntiles, int i_first, int nrow_tiles, int B, TilePat pat, HBlk hb) {
  using E = Engine<double>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* smem = reinterpret_cast<double*>(smem_raw);
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int b8 = gridDim.x / (8 * nrow_tiles);       // (the two block maps: chol_offdiag_f32_kernel)
  const int b = pat.lpt ? (slot % b8) * 8 + xcd : (slot / nrow_tiles) * 8 + xcd;
  const int rslot = pat.lpt ? slot / b8 : slot % nrow_tiles;
  // (tile-sparse: i_first = first ENTRY of the launch, relative to the column's list -- level schedule: absolute, and the entry
  //  names its block column)
  const int ent = pat.col_row ? (pat.ent_col ? 0 : pat.col_ptr[jarg]) + i_first + rslot : 0;
  // (right-looking schedule, TilePat.rl: see chol_offdiag_f32_kernel)
  const bool combo = RL && pat.rl_nsub > 0;
  const bool upd = RL && (combo ? rslot >= pat.rl_nsub : pat.rl >= 2);
  const int jc = combo ? jarg - 1 : pat.rl - 2;
  const int ub = combo ? jarg + 1 : jc + 1;
  const bool sla = RL && pat.rl == 1 && pat.rl_la != 0;
  int ui = 0, uk = 0;
  if (RL && upd) {   // (i_first: the launch's first slot, see chol_offdiag_f32_kernel)
    const int us = combo ? rslot - pat.rl_nsub : rslot + i_first;
    ui = (int)((__builtin_sqrtf(8.f * (float)us + 1.f) - 1.f) * 0.5f);
    while ((ui + 1) * (ui + 2) / 2 <= us) ++ui;
    while (ui * (ui + 1) / 2 > us) --ui;
    uk = us - ui * (ui + 1) / 2;
  }
  const int j = upd ? ub + uk : (pat.ent_col ? pat.ent_col[ent] : jarg);
  const int i = upd ? ub + ui : (pat.col_row ? pat.col_row[ent] : i_first + rslot);
  const int32_t* klist = pat.col_row ? pat.tile_k + pat.tile_kptr[ent] : nullptr;
  const int Kspan = (RL && pat.rl) ? ((upd || sla) ? TILE : 0) : (pat.col_row ? (pat.tile_kptr[ent + 1] - pat.tile_kptr[ent]) * TILE : j * TILE);
  const int kcol0 = upd ? jc * TILE : (sla ? (jarg - 1) * TILE : 0);
  if (b >= B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rl = lane & 15, kq = lane >> 4;
  const LFrame lf = lframe(pat, ld);
  const int64_t mat = (int64_t)b * ld * ld;            // H (dense frame)
  const int64_t lmat = (int64_t)b * lf.pstride;        // L (dense frame or tile-packed)
  const int64_t ldt = lf.ld;
  double* const Lij = L + lmat + lf.tile(i, j, ntiles + ent);
  const int32_t* ksa = lf.packed ? pat.tile_sa + pat.tile_kptr[ent] : nullptr;
  const int32_t* ksb = lf.packed ? pat.tile_sb + pat.tile_kptr[ent] : nullptr;
  const int col0 = j * TILE, row0 = i * TILE;
  const int validB = tile_rows(pat, n, i);
  double* sA = smem;
  double* sB = smem + 128 * CT<double>::LDT;

  E::Acc P;
  E::zero(P);
  HBPre<double, HB ? HB_NPRE_OFF : 1> hbp;
  if constexpr (HB) hbp.load(hb, b, i, j, tid);
  // panel sub-block q (row-major list of the lower triangle): block row SB[q], block column TB[q]
  const double* Pn = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
  double* const smemE = smem + OFF64_STAGE / 8;
  // sub-blocks 0..4 -> E by LDS-direct loads: lane l of wave w, pass u writes the 16-byte unit U = 256 u + 64 w + l of the block
  // (row r = U / 16, unit u' = U % 16) and fetches the unit u' ^ (r & 15) of that row -- the XOR swizzle sub_mma64 reads with
  auto prefetch_panel = [&]() __attribute__((always_inline)) {
    if (upd) return;   // (trailing update: no substitution, no panel)
    constexpr int SB[5] = {0, 1, 1, 2, 2}, TB[5] = {0, 0, 1, 0, 1};
#pragma unroll
    for (int q = 0; q < OFF64_EBLK; ++q)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int U = 256 * u + 64 * wave + lane, r = U >> 4, up = U & 15;
        const double* src = Pn + (32 * SB[q] + r) * TILE + 32 * TB[q] + 2 * (up ^ (r & 15));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(smemE + q * 1024 + (256 * u + 64 * wave) * 2),
                                         16, 0, 0);
      }
  };
  kloop<double, false>(L + lmat + (lf.packed ? 0 : (int64_t)col0 * ld) + kcol0, upd ? tile_rows(pat, n, j) : TILE,
                       L + lmat + (lf.packed ? 0 : (int64_t)row0 * ld) + kcol0, validB,
                       ldt, Kspan, sA, sB, P, tid, nullptr, nullptr, prefetch_panel, klist, ksa, ksb, lf.pstride);
  // sub-blocks 5..8 go LDS-direct into the staging buffers as soon as those are free (dense H: now, next to the H loads;
  // block-compact H: after the gather rounds), W_33 (sub-block 9) LDS-direct into sub-block 0's place in E once E has been read.
  // No panel data in registers: round 4 parked sub-blocks 5..9 (block-compact H) / W_33 (dense H) in VGPRs from here on and
  // hipcc spilled them -- 160 B per thread through scratch, 1 GB of extra HBM traffic per launch (profiles/r5/ab_, ac_).
  if (!HB && !upd) {
    // dense H: 5..8 straight into the staging buffers (LDS-direct, no registers: the 128 VGPRs of the H tile are about to be in
    // flight) -- after a barrier: the K-loop ends on a chunk's MFMAs, a slower wave may still be reading its fragments
    __syncthreads();
    constexpr int SB[4] = {2, 3, 3, 3}, TB[4] = {2, 0, 1, 2};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int U = 256 * u + 64 * wave + lane, r = U >> 4, up = U & 15;
        const double* src = Pn + (32 * SB[q] + r) * TILE + 32 * TB[q] + 2 * (up ^ (r & 15));
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(smem + q * 1024 + (256 * u + 64 * wave) * 2),
                                         16, 0, 0);
      }
  }
  // one panel sub-block (block row sbr, block column sbc) -> LDS at dst, LDS-direct, in sub_mma64's swizzled layout
  auto panel_dma = [&](int sbr, int sbc, double* dst) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int U = 256 * u + 64 * wave + lane, r = U >> 4, up = U & 15;
      const double* src = Pn + (32 * sbr + r) * TILE + 32 * sbc + 2 * (up ^ (r & 15));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + (256 * u + 64 * wave) * 2), 16, 0, 0);
    }
  };
  if constexpr (HB) {
    // block-compact H: the tile's pieces through the (free) staging buffers, 32 rows -- one wave's -- at a time
    constexpr int LDH = 130;
    static_assert(32 * LDH * 8 <= OFF64_STAGE, "a quarter of an H tile must fit in the staging buffers");
    __syncthreads();
    // P = -sum first, H_ij's pieces are ADDED
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) P.v[h][cb][rho] = -P.v[h][cb][rho];
    if constexpr (HB == HB_MODE_SCATTER) {
      // a few pieces per tile (pose graphs): added by the matrix cores, see hb_scatter
      static_assert((256 * HB_NPRE_OFF + 64 * 36) * 8 <= OFF64_STAGE, "list + overflow chunk inside the staging buffers");
      hb_add<double, E::Acc, decltype(hbp), 256 * HB_NPRE_OFF>(P, hbp, hb, b, smem, 0, hbp.cnt / (hb.bd * hb.bd), true, tid);
      __syncthreads();   // the list has been read: panel sub-blocks 5..8 may take the staging buffers
    } else {
#pragma unroll
    for (int rd = 0; rd < 4; ++rd) {
      for (int k = tid; k < 32 * LDH / 2; k += 256) reinterpret_cast<double2*>(smem)[k] = make_double2(0.0, 0.0);
      __syncthreads();
      hbp.foreach(hb, b, tid, [&](int rr, int cc, double v) __attribute__((always_inline)) {
        if ((rr >> 5) == rd) smem[(rr & 31) * LDH + cc] = v;
      });
      __syncthreads();
      if (wave == rd) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double* hrow = smem + (16 * h + rl) * LDH + kq;
#pragma unroll
          for (int cb = 0; cb < 8; ++cb)
#pragma unroll
            for (int rho = 0; rho < 4; ++rho) P.v[h][cb][rho] = hrow[16 * cb + 4 * rho] + P.v[h][cb][rho];   // (P holds -sum already)
        }
      }
      __syncthreads();
    }
    }
  } else {
  // ---- P = H_ij - sum, H straight from global memory in the native layout (rows outside the matrix: zero) ----
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = 32 * wave + 16 * h + rl;
    const bool rv = r < validB;
    const double* Hrow = H + mat + (int64_t)(row0 + (rv ? r : 0)) * ld + col0 + kq;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const double hv = Hrow[16 * cb + 4 * rho];
        P.v[h][cb][rho] = (rv ? hv : 0.0) - P.v[h][cb][rho];
      }
  }
  }
  if (RL && upd) {   // trailing update: the tile goes back as it is (a diagonal tile: its lower triangle, zeros above)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 32 * wave + 16 * h + rl;
      if (r < validB) {
        double* Lrow = Lij + (int64_t)r * ldt + kq;
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
#pragma unroll
          for (int rho = 0; rho < 4; ++rho) {
            const int c = 16 * cb + 4 * rho + kq;
            Lrow[16 * cb + 4 * rho] = (i == j && c > r) ? 0.0 : P.v[h][cb][rho];
          }
      }
    }
    return;
  }
  if constexpr (HB) {
    // sub-blocks 5..8 -> the staging buffers, LDS-direct, now that the gather rounds are done with them (their last barrier has
    // passed); they land under the first five block products, which read E.  E itself was requested in the prologue: every wave
    // has waited for its own pieces inside the K-loop (older loads) -- or right here when the K-loop was empty -- and the gather's
    // barriers published them.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (Kspan == 0) __syncthreads();
    panel_dma(2, 2, smem + 0 * 1024);
    panel_dma(3, 0, smem + 1 * 1024);
    panel_dma(3, 1, smem + 2 * 1024);
    panel_dma(3, 2, smem + 3 * 1024);
  } else {
    // E (LDS-direct loads of the prologue) and the staging buffers complete and visible to every wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  // ---- in-place substitution ----
  auto solve_diag = [&](auto is, const double* Wss) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value;
    f64x4 T0[2], T1[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) { T0[h][r4] = 0.0; T1[h][r4] = 0.0; }
    sub_mma64<sb, sb>(Wss, P, T0, T1, lane);  // X_s = W_ss P_s
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      P.v[h][2 * sb] = T0[h];
      P.v[h][2 * sb + 1] = T1[h];
    }
  };
  auto update = [&](auto is, auto it, const double* Mst) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value, tb = decltype(it)::value;
    f64x4 D0[2] = {P.v[0][2 * sb], P.v[1][2 * sb]}, D1[2] = {P.v[0][2 * sb + 1], P.v[1][2 * sb + 1]};
    sub_mma64<sb, tb>(Mst, P, D0, D1, lane);  // P_s += (-L_st) X_t  (X_t lives in P_t's registers)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      P.v[h][2 * sb] = D0[h];
      P.v[h][2 * sb + 1] = D1[h];
    }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  // sub-blocks 0..4 from E (there since the first k-chunk)
  solve_diag(I0{}, smemE + 0 * 1024);
  update(I1{}, I0{}, smemE + 1 * 1024);
  solve_diag(I1{}, smemE + 2 * 1024);
  update(I2{}, I0{}, smemE + 3 * 1024);
  update(I2{}, I1{}, smemE + 4 * 1024);
  if constexpr (HB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // sub-blocks 5..8 (LDS-direct) and W_33 have landed
  __syncthreads();                  // every wave is done with E (block-compact H: and sees sub-blocks 5..8)
  panel_dma(3, 3, smemE + 0 * 1024);   // sub-block 9 = W_33 takes sub-block 0's place: LDS-direct, lands under the next four block
                                       // products (round 4 parked it in 8 VGPRs from the K-loop's end on: spilled to scratch)
  solve_diag(I2{}, smem + 0 * 1024);
  update(I3{}, I0{}, smem + 1 * 1024);
  update(I3{}, I1{}, smem + 2 * 1024);
  update(I3{}, I2{}, smem + 3 * 1024);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                  // W_33 in place
  solve_diag(I3{}, smemE + 0 * 1024);
  // ---- store X (in P's registers) ----
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = 32 * wave + 16 * h + rl;
    if (r < validB) {
      double* Lrow = Lij + (int64_t)r * ldt + kq;
#pragma unroll
      for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) Lrow[16 * cb + 4 * rho] = P.v[h][cb][rho];
    }
  }
  if (RL && pat.rl_y) {   // right-looking forward substitution: block i of the vector loses L_ij y_j (a row's 128 columns sit in four lanes)
    double* yb = static_cast<double*>(pat.rl_y) + (int64_t)b * pat.rl_ldv;
    const double* yj = yb + col0 + kq;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double dot = 0.0;
#pragma unroll
      for (int cb = 0; cb < 8; ++cb)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) dot += P.v[h][cb][rho] * yj[16 * cb + 4 * rho];
      dot += __shfl_xor(dot, 16);
      dot += __shfl_xor(dot, 32);
      const int r = 32 * wave + 16 * h + rl;
      if (kq == 0 && r < validB) yb[row0 + r] -= dot;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// chol_offdiag, fp64, EIGHT waves per workgroup (round 6): the same tile, staging, panel plan and arithmetic -- element by element
// the same sequence of MFMAs, bit-identical results -- with a wave owning 16 rows x 128 columns instead of 32 x 128: 64 accumulator
// VGPRs, <= 128 in all, two workgroups = FOUR waves per SIMD.  Why: the 4-wave kernel is two waves per SIMD (256 VGPRs); with
// K-loops of zero to three tiles -- block columns 0 ... 3, 27 of the 95 ms -- a tile's time is its serial epilogue (H pieces, ten
// dependent block products of the substitution, 128 KB of stores), which one other wave per SIMD cannot cover: 0.39 ... 0.71 of
// the peak per executed flop (profiles/r5/x_).  Half the epilogue per wave and twice the waves to interleave.  MEASURED
// (profiles/r6/ae_): the early columns gain NOTHING (their tiles are serial phases -- pieces, panel waits, ten dependent block
// products, stores -- that more waves of the SAME tile do not overlap; it takes more TILES per CU), the late ones 0.1 - 0.3 ms
// each: 91.5 -> 90.4 ms with every column on this kernel, which is the default.  Left-looking column schedule only (no TilePat.rl
// modes, no tile pattern); block-compact H through the matrix-core scatter or a dense H frame (HB_MODE_ROUNDS: the 4-wave kernel).
// ------------------------------------------------------------------------------------------------
template <int S, int Tt>
__device__ __forceinline__ void sub_mma64_16(const double* blk, const Acc16& Bs, f64x4& D0, f64x4& D1, int lane) {
  const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
#pragma unroll
    for (int cbh = 0; cbh < 2; ++cbh)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const int r = 16 * ch + rl, c = 16 * cbh + 4 * rho + kq;
        const double a = blk[r * 32 + (c ^ (2 * rl))];
        auto& d = ch == 0 ? D0 : D1;
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs.v[2 * Tt + cbh][rho], d, 0, 0, 0);
      }
}

template <int HB>
__global__ void __launch_bounds__(512, 4)   // (second argument: waves per SIMD -- two workgroups of eight per CU)
chol_offdiag_f64w8_kernel(const double* __restrict__ H, double* __restrict__ L, const double* __restrict__ panel, int n,
                          int64_t ld, int jarg, int ntiles, int i_first, int nrow_tiles, int B, TilePat pat, HBlk hb) {
  static_assert(HB != HB_MODE_ROUNDS, "dense tiles of H: the 4-wave kernel");
  constexpr int NT = 512;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* smem = reinterpret_cast<double*>(smem_raw);
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int b8 = gridDim.x / (8 * nrow_tiles);       // (the two block maps: chol_offdiag_f32_kernel)
  const int b = pat.lpt ? (slot % b8) * 8 + xcd : (slot / nrow_tiles) * 8 + xcd;
  const int rslot = pat.lpt ? slot / b8 : slot % nrow_tiles;
  const int ent = pat.col_row ? (pat.ent_col ? 0 : pat.col_ptr[jarg]) + i_first + rslot : 0;
  const int j = pat.ent_col ? pat.ent_col[ent] : jarg;
  const int i = pat.col_row ? pat.col_row[ent] : i_first + rslot;
  const int32_t* klist = pat.col_row ? pat.tile_k + pat.tile_kptr[ent] : nullptr;
  const int Kspan = pat.col_row ? (pat.tile_kptr[ent + 1] - pat.tile_kptr[ent]) * TILE : j * TILE;
  if (b >= B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rl = lane & 15, kq = lane >> 4;
  const LFrame lf = lframe(pat, ld);
  const int64_t mat = (int64_t)b * ld * ld;
  const int64_t lmat = (int64_t)b * lf.pstride;
  const int64_t ldt = lf.ld;
  double* const Lij = L + lmat + lf.tile(i, j, ntiles + ent);
  const int32_t* ksa = lf.packed ? pat.tile_sa + pat.tile_kptr[ent] : nullptr;
  const int32_t* ksb = lf.packed ? pat.tile_sb + pat.tile_kptr[ent] : nullptr;
  const int col0 = j * TILE, row0 = i * TILE;
  const int validB = tile_rows(pat, n, i);
  double* sA = smem;
  double* sB = smem + 128 * CT<double>::LDT;
  Acc16 P;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int k = 0; k < 4; ++k) P.v[cb][k] = 0.0;
  HBPre<double, HB ? 2 : 1, NT> hbp;
  if constexpr (HB != 0) hbp.load(hb, b, i, j, tid);
  const double* Pn = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
  double* const smemE = smem + OFF64_STAGE / 8;
  // one panel sub-block (block row sbr, block column sbc) -> LDS at dst, LDS-direct, in sub_mma64's swizzled layout: thread U
  // writes the 16-byte unit U of the block (row r = U / 16, unit U % 16) and fetches the unit (U % 16) ^ (r & 15) of that row
  auto panel_dma = [&](int sbr, int sbc, double* dst) __attribute__((always_inline)) {
    const int U = tid, r = U >> 4, up = U & 15;
    const double* src = Pn + (32 * sbr + r) * TILE + 32 * sbc + 2 * (up ^ (r & 15));
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)(dst + (64 * wave) * 2), 16, 0, 0);
  };
  auto prefetch_panel = [&]() __attribute__((always_inline)) {   // sub-blocks 0..4 -> E (chol_offdiag_f64_kernel)
    panel_dma(0, 0, smemE + 0 * 1024);
    panel_dma(1, 0, smemE + 1 * 1024);
    panel_dma(1, 1, smemE + 2 * 1024);
    panel_dma(2, 0, smemE + 3 * 1024);
    panel_dma(2, 1, smemE + 4 * 1024);
  };
  {
    const double* sBw = sB + 16 * wave * CT<double>::LDT;
    kloop_f<double, false, false, CT<double>::LDT, false, NT>(
        L + lmat + (lf.packed ? 0 : (int64_t)col0 * ld), TILE, L + lmat + (lf.packed ? 0 : (int64_t)row0 * ld), validB, ldt, Kspan, sA,
        sB, tid, nullptr, nullptr,
        [&]() __attribute__((always_inline)) {
          constexpr int LDT = CT<double>::LDT;
#pragma unroll
          for (int ks = 0; ks < CT<double>::KB / 8; ++ks) {
            const double2 fb = *reinterpret_cast<const double2*>(sBw + rl * LDT + 8 * ks + 2 * kq);
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
              const double2 fa = *reinterpret_cast<const double2*>(sA + (16 * cb + rl) * LDT + 8 * ks + 2 * kq);
              P.v[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.x, fb.x, P.v[cb], 0, 0, 0);
              P.v[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.y, fb.y, P.v[cb], 0, 0, 0);
            }
          }
        },
        prefetch_panel, klist, ksa, ksb, lf.pstride);
  }
  const int r = 16 * wave + rl;   // this lane's tile row
  if constexpr (HB == 0) {
    // dense H: sub-blocks 5..8 straight into the staging buffers (after a barrier: a slower wave may still read its fragments)
    __syncthreads();
    panel_dma(2, 2, smem + 0 * 1024);
    panel_dma(3, 0, smem + 1 * 1024);
    panel_dma(3, 1, smem + 2 * 1024);
    panel_dma(3, 2, smem + 3 * 1024);
    const bool rv = r < validB;
    const double* Hrow = H + mat + (int64_t)(row0 + (rv ? r : 0)) * ld + col0 + kq;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const double hv = Hrow[16 * cb + 4 * rho];
        P.v[cb][rho] = (rv ? hv : 0.0) - P.v[cb][rho];
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();   // E and the staging buffers complete and visible to every wave
  } else {
    __syncthreads();   // the K-loop's last chunk has been consumed: the staging buffers are free
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) P.v[cb][rho] = -P.v[cb][rho];
    static_assert((NT * 2 + 64 * 36) * 8 <= OFF64_STAGE, "list + overflow chunk inside the staging buffers");
    hb_add<double, Acc16, decltype(hbp), NT * 2, NT>(P, hbp, hb, b, smem, 0, hbp.cnt / (hb.bd * hb.bd), true, tid);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of E (requested in the prologue) have landed
    __syncthreads();   // the list has been read; E visible to every wave (also when the K-loop was empty)
    panel_dma(2, 2, smem + 0 * 1024);   // sub-blocks 5..8: they land under the first five block products, which read E
    panel_dma(3, 0, smem + 1 * 1024);
    panel_dma(3, 1, smem + 2 * 1024);
    panel_dma(3, 2, smem + 3 * 1024);
  }
  // ---- in-place substitution (chol_offdiag_f64_kernel's, on 16 rows) ----
  auto solve_diag = [&](auto is, const double* Wss) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value;
    f64x4 T0, T1;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) { T0[r4] = 0.0; T1[r4] = 0.0; }
    sub_mma64_16<sb, sb>(Wss, P, T0, T1, lane);  // X_s = W_ss P_s
    P.v[2 * sb] = T0;
    P.v[2 * sb + 1] = T1;
  };
  auto update = [&](auto is, auto it, const double* Mst) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value, tb = decltype(it)::value;
    sub_mma64_16<sb, tb>(Mst, P, P.v[2 * sb], P.v[2 * sb + 1], lane);  // P_s += (-L_st) X_t
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  solve_diag(I0{}, smemE + 0 * 1024);
  update(I1{}, I0{}, smemE + 1 * 1024);
  solve_diag(I1{}, smemE + 2 * 1024);
  update(I2{}, I0{}, smemE + 3 * 1024);
  update(I2{}, I1{}, smemE + 4 * 1024);
  if constexpr (HB != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // sub-blocks 5..8 have landed
  __syncthreads();                       // every wave is done with E (block-compact H: and sees sub-blocks 5..8)
  panel_dma(3, 3, smemE + 0 * 1024);     // W_33 takes sub-block 0's place, lands under the next four block products
  solve_diag(I2{}, smem + 0 * 1024);
  update(I3{}, I0{}, smem + 1 * 1024);
  update(I3{}, I1{}, smem + 2 * 1024);
  update(I3{}, I2{}, smem + 3 * 1024);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                       // W_33 in place
  solve_diag(I3{}, smemE + 0 * 1024);
  // ---- store X ----
  if (r < validB) {
    double* Lrow = Lij + (int64_t)r * ldt + kq;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) Lrow[16 * cb + 4 * rho] = P.v[cb][rho];
  }
}

// ------------------------------------------------------------------------------------------------
// chol_offdiag, fp64, HALF TILES (round 6): a workgroup of four waves produces 64 rows x 128 columns of the tile (16 rows
// per wave, Acc16), with 36.8 KB of LDS -- the K-loop's staging buffers and nothing else -- and <= 128 VGPRs: FOUR workgroups per CU
// instead of two.  For the block columns with K-loops of zero to three tiles, whose tiles are chains of latency-bound phases (pieces
// of H, panel waits, ten dependent block products, stores) that two resident workgroups cannot overlap.  The price: each half
// stages the whole column panel L_j (1.5x the operand traffic per tile product), the solve panel is not prefetched under the K-loop
// but fetched afterwards, four sub-blocks at a time into the free staging buffers (three exposed round trips), one k-chunk in
// flight instead of two.  Same MFMAs in the same order per element: bit-identical (tests/test_gpu_block_hessian.py).
// MEASURED (profiles/r6/af_): n = 1536, batch 4096: 90.0 -> 88.5 ms with the first 6 - 8 block columns on this kernel (0.700 -> 0.711),
// every further column gives 0.1 ms back (the K-loop with one chunk in flight and 1.5x the staging loses to the 8-wave kernel from
// ~8 tiles on): thx_chol_schedule.f64_half_max_ktiles, default 8.
// ------------------------------------------------------------------------------------------------
constexpr int F64H_AHEAD = 1;   // k-chunks in flight (2: 142 VGPRs wanted, spills -- see the header comment)
template <int HB>
__global__ void __launch_bounds__(256, 4)
chol_offdiag_f64h_kernel(const double* __restrict__ H, double* __restrict__ L, const double* __restrict__ panel, int n,
                         int64_t ld, int jarg, int ntiles, int i_first, int nrow_tiles, int B, TilePat pat, HBlk hb) {
  static_assert(HB != HB_MODE_ROUNDS, "dense tiles of H: the 4-wave full-tile kernel");
  constexpr int NT = 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* smem = reinterpret_cast<double*>(smem_raw);
  const int bid = blockIdx.x;
  const int xcd = bid & 7, slot = bid >> 3;
  const int nslots = 2 * nrow_tiles;                 // (two halves per row tile, adjacent slots)
  const int b = (slot / nslots) * 8 + xcd;
  const int hslot = slot % nslots;
  const int half = hslot & 1, rslot = hslot >> 1;
  const int j = jarg, i = i_first + rslot;
  const int Kspan = j * TILE;
  if (b >= B) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int rl = lane & 15, kq = lane >> 4;
  const int64_t mat = (int64_t)b * ld * ld;
  const int col0 = j * TILE, row0 = i * TILE + 64 * half;
  const int validB = min(64, tile_rows(pat, n, i) - 64 * half);   // rows of this half inside the matrix
  if (validB <= 0) return;
  double* const Lij = L + mat + (int64_t)row0 * ld + col0;
  double* sA = smem;
  double* sB = smem + 128 * CT<double>::LDT;
  Acc16 P;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int k = 0; k < 4; ++k) P.v[cb][k] = 0.0;
  HBPre<double, HB ? HB_NPRE_OFF : 1, NT> hbp;
  if constexpr (HB != 0) hbp.load(hb, b, i, j, tid);
  const double* Pn = panel + ((int64_t)b * ntiles + j) * TILE * TILE;
  {
    const double* sBw = sB + 16 * wave * CT<double>::LDT;
    kloop_f<double, false, false, CT<double>::LDT, false, NT, F64H_AHEAD, 64>(
        L + mat + (int64_t)col0 * ld, TILE, L + mat + (int64_t)row0 * ld, validB, ld, Kspan, sA, sB, tid, nullptr, nullptr,
        [&]() __attribute__((always_inline)) {
          constexpr int LDT = CT<double>::LDT;
#pragma unroll
          for (int ks = 0; ks < CT<double>::KB / 8; ++ks) {
            const double2 fb = *reinterpret_cast<const double2*>(sBw + rl * LDT + 8 * ks + 2 * kq);
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
              const double2 fa = *reinterpret_cast<const double2*>(sA + (16 * cb + rl) * LDT + 8 * ks + 2 * kq);
              P.v[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.x, fb.x, P.v[cb], 0, 0, 0);
              P.v[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.y, fb.y, P.v[cb], 0, 0, 0);
            }
          }
        });
  }
  const int r = 16 * wave + rl;   // this lane's row inside the half
  __syncthreads();                // the K-loop's last chunk has been consumed: the staging buffers are free
  if constexpr (HB == 0) {
    const bool rv = r < validB;
    const double* Hrow = H + mat + (int64_t)(row0 + (rv ? r : 0)) * ld + col0 + kq;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const double hv = Hrow[16 * cb + 4 * rho];
        P.v[cb][rho] = (rv ? hv : 0.0) - P.v[cb][rho];
      }
  } else {
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) P.v[cb][rho] = -P.v[cb][rho];
    static_assert((NT * HB_NPRE_OFF + 64 * 36) * 8 <= OFF64_STAGE, "list + overflow chunk inside the staging buffers");
    // (hb_scatter's "wave" names the 16-row block of the TILE: 4 half + wave)
    {
      const int bd = hb.bd, bb = bd * bd;
      const int nreg = min(min(hbp.cnt / bb, NT * HB_NPRE_OFF / bb), 64), np = hbp.cnt / bb;
      const int wv = __builtin_amdgcn_readfirstlane(4 * half + wave);
      hbp.to_list(smem, tid);
      __syncthreads();
      hb_scatter(P, smem, hbp.wmeta, 0, nreg, bd, wv, lane);
      if (np > nreg) {   // (workgroup uniform) crowded tile: further chunks of 64 pieces from memory (hb_add)
        const double* base = static_cast<const double*>(hb.blocks) + (int64_t)b * hb.bstride;
        double* over = smem + NT * HB_NPRE_OFF;
        for (int q0 = nreg; q0 < np; q0 += 64) {
          const int nq = min(64, np - q0);
          __syncthreads();
          for (int idx = tid; idx < nq * bb; idx += NT) over[idx] = base[(int64_t)hb.piece_blk[hbp.p0 + q0 + idx / bb] * bb + idx % bb];
          const int wm = hb.piece_rc[hbp.p0 + q0 + min(lane, nq - 1)];
          __syncthreads();
          hb_scatter(P, over, wm, 0, nq, bd, wv, lane);
        }
      }
    }
    __syncthreads();   // the list has been read: the panel may take the staging buffers
  }
  // one panel sub-block -> LDS slot, LDS-direct, in sub_mma64's swizzled layout (two passes of the 256 threads)
  auto panel_dma = [&](int sbr, int sbc, double* dst) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int U = 256 * u + tid, rr = U >> 4, up = U & 15;
      const double* src = Pn + (32 * sbr + rr) * TILE + 32 * sbc + 2 * (up ^ (rr & 15));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(dst + (256 * u + 64 * wave) * 2), 16, 0, 0);
    }
  };
  auto landed = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  };
  auto solve_diag = [&](auto is, const double* Wss) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value;
    f64x4 T0, T1;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) { T0[r4] = 0.0; T1[r4] = 0.0; }
    sub_mma64_16<sb, sb>(Wss, P, T0, T1, lane);
    P.v[2 * sb] = T0;
    P.v[2 * sb + 1] = T1;
  };
  auto update = [&](auto is, auto it, const double* Mst) __attribute__((always_inline)) {
    constexpr int sb = decltype(is)::value, tb = decltype(it)::value;
    sub_mma64_16<sb, tb>(Mst, P, P.v[2 * sb], P.v[2 * sb + 1], lane);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  // ---- the substitution in three panel phases of four / four / two sub-blocks through the staging buffers (each an exposed round
  //      trip, covered by the other three workgroups of the CU) ----
  panel_dma(0, 0, smem + 0 * 1024);
  panel_dma(1, 0, smem + 1 * 1024);
  panel_dma(1, 1, smem + 2 * 1024);
  panel_dma(2, 0, smem + 3 * 1024);
  landed();
  solve_diag(I0{}, smem + 0 * 1024);
  update(I1{}, I0{}, smem + 1 * 1024);
  solve_diag(I1{}, smem + 2 * 1024);
  update(I2{}, I0{}, smem + 3 * 1024);
  __syncthreads();   // every wave is done with the four slots
  panel_dma(2, 1, smem + 0 * 1024);
  panel_dma(2, 2, smem + 1 * 1024);
  panel_dma(3, 0, smem + 2 * 1024);
  panel_dma(3, 1, smem + 3 * 1024);
  landed();
  update(I2{}, I1{}, smem + 0 * 1024);
  solve_diag(I2{}, smem + 1 * 1024);
  update(I3{}, I0{}, smem + 2 * 1024);
  update(I3{}, I1{}, smem + 3 * 1024);
  __syncthreads();
  panel_dma(3, 2, smem + 0 * 1024);
  panel_dma(3, 3, smem + 1 * 1024);
  landed();
  update(I3{}, I2{}, smem + 0 * 1024);
  solve_diag(I3{}, smem + 1 * 1024);
  // ---- store X ----
  if (r < validB) {
    double* Lrow = Lij + (int64_t)r * ld + kq;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) Lrow[16 * cb + 4 * rho] = P.v[cb][rho];
  }
}

}  // namespace thx
