#pragma once
#include "common.cuh"
#include "chol_base.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// K-loop engines.  Stage rows through LDS (register prefetch of the next chunk), accumulate
// acc[r][c] = sum_k Brows[r][k] * Arows[c][k] in the transposed MFMA layout.
// ------------------------------------------------------------------------------------------------
template <typename T>
struct Engine;

template <>
struct Engine<float> {
  struct Acc {
    f32x16 v[4];
  };
  static __device__ __forceinline__ void zero(Acc& a) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) a.v[i][j] = 0.f;
  }
  static __device__ __forceinline__ void chunk(const float* sA, const float* sBw, Acc& acc, int lane) {
    const int rl = lane & 31, g = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float4 fb = *reinterpret_cast<const float4*>(sBw + rl * 36 + 8 * ks + 4 * g);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const float4 fa = *reinterpret_cast<const float4*>(sA + (32 * cb + rl) * 36 + 8 * ks + 4 * g);
        acc.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc.v[cb], 0, 0, 0);
        acc.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc.v[cb], 0, 0, 0);
        acc.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc.v[cb], 0, 0, 0);
        acc.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc.v[cb], 0, 0, 0);
      }
    }
  }

  // SYRK of the diagonal tile on the 36 lower 16x16 blocks of its 8x8 block grid, nine per wave: wave g owns block
  // rows 4+g (5+g blocks) and 3-g (4-g blocks) -- equal MFMA counts on all four SIMDs, 56 % of the full tile.
  // v_mfma_f32_16x16x4_f32.  Staged rows have stride SYRK_LDT = 40 words and lane (r, kq) reads the two 16-byte
  // pieces at words 4kq and 16+4kq (an MFMA's k index is only a pairing of columns): the one (stride, offsets)
  // combination for which the ds_read_b128 of a 16x16 fragment is bank-conflict free (stride 36: 32 % conflicts).
  static constexpr int SYRK_LDT = 40;
  static constexpr int SYRK_STAGE = 128 * SYRK_LDT;   // elements of the SYRK K-loop's staging buffer
  using Sy = f32x4;
  template <int G>
  static __device__ __forceinline__ void syrk36(const float* sA, f32x4* acc, int lane) {
    constexpr int UH = 4 + G, UL = 3 - G;
    const int o = (lane & 15) * 40 + 4 * (lane >> 4);
    float fbh[8], fbl[8];
    {
      const float4 a = *reinterpret_cast<const float4*>(sA + 16 * UH * 40 + o), b = *reinterpret_cast<const float4*>(sA + 16 * UH * 40 + o + 16);
      const float4 c = *reinterpret_cast<const float4*>(sA + 16 * UL * 40 + o), d = *reinterpret_cast<const float4*>(sA + 16 * UL * 40 + o + 16);
      fbh[0] = a.x; fbh[1] = a.y; fbh[2] = a.z; fbh[3] = a.w; fbh[4] = b.x; fbh[5] = b.y; fbh[6] = b.z; fbh[7] = b.w;
      fbl[0] = c.x; fbl[1] = c.y; fbl[2] = c.z; fbl[3] = c.w; fbl[4] = d.x; fbl[5] = d.y; fbl[6] = d.z; fbl[7] = d.w;
    }
#pragma unroll
    for (int v = 0; v <= UH; ++v) {
      float fa[8];
      if (v == UH) {
#pragma unroll
        for (int m = 0; m < 8; ++m) fa[m] = fbh[m];
      } else if (v == UL) {
#pragma unroll
        for (int m = 0; m < 8; ++m) fa[m] = fbl[m];
      } else {
        const float4 a = *reinterpret_cast<const float4*>(sA + 16 * v * 40 + o), b = *reinterpret_cast<const float4*>(sA + 16 * v * 40 + o + 16);
        fa[0] = a.x; fa[1] = a.y; fa[2] = a.z; fa[3] = a.w; fa[4] = b.x; fa[5] = b.y; fa[6] = b.z; fa[7] = b.w;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) acc[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[m], fbh[m], acc[v], 0, 0, 0);
      if (v <= UL) {
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[UH + 1 + v] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[m], fbl[m], acc[UH + 1 + v], 0, 0, 0);
      }
    }
  }
  // syrk36 on SORTED staged rows (chol_syrk_kernel<float, true, true>): ``m`` names the chunk's active block rows (wave uniform); block
  // (u, v) runs only when both its block rows are active, with the same MFMA sequence as above, and the fragments of an inactive
  // block row are not read (its LDS rows hold stale data).
  template <int G>
  static __device__ __forceinline__ void syrk36_masked(const float* sA, f32x4* acc, int lane, int m) {
    constexpr int UH = 4 + G, UL = 3 - G;
    const bool hh = (m >> UH) & 1, hl = (m >> UL) & 1;
    if (!hh && !hl) return;
    const int o = (lane & 15) * 40 + 4 * (lane >> 4);
    float fbh[8], fbl[8];   // (read only where loaded)
    if (hh) {
      const float4 a = *reinterpret_cast<const float4*>(sA + 16 * UH * 40 + o), b = *reinterpret_cast<const float4*>(sA + 16 * UH * 40 + o + 16);
      fbh[0] = a.x; fbh[1] = a.y; fbh[2] = a.z; fbh[3] = a.w; fbh[4] = b.x; fbh[5] = b.y; fbh[6] = b.z; fbh[7] = b.w;
    }
    if (hl) {
      const float4 c = *reinterpret_cast<const float4*>(sA + 16 * UL * 40 + o), d = *reinterpret_cast<const float4*>(sA + 16 * UL * 40 + o + 16);
      fbl[0] = c.x; fbl[1] = c.y; fbl[2] = c.z; fbl[3] = c.w; fbl[4] = d.x; fbl[5] = d.y; fbl[6] = d.z; fbl[7] = d.w;
    }
#pragma unroll
    for (int v = 0; v <= UH; ++v) {
      if (!((m >> v) & 1)) continue;
      const bool lo = v <= UL && hl;
      if (!hh && !lo) continue;
      float fa[8];
      if (v == UH) {
#pragma unroll
        for (int q = 0; q < 8; ++q) fa[q] = fbh[q];
      } else if (v == UL) {
#pragma unroll
        for (int q = 0; q < 8; ++q) fa[q] = fbl[q];
      } else {
        const float4 a = *reinterpret_cast<const float4*>(sA + 16 * v * 40 + o), b = *reinterpret_cast<const float4*>(sA + 16 * v * 40 + o + 16);
        fa[0] = a.x; fa[1] = a.y; fa[2] = a.z; fa[3] = a.w; fa[4] = b.x; fa[5] = b.y; fa[6] = b.z; fa[7] = b.w;
      }
      if (hh) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[q], fbh[q], acc[v], 0, 0, 0);
      }
      if (lo) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[UH + 1 + v] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[q], fbl[q], acc[UH + 1 + v], 0, 0, 0);
      }
    }
  }
  // The same nine blocks of H_jj, global -> registers BEFORE the K-loop (row index clamped into the matrix: the caller
  // masks by value), so that the H tile costs no exposed round trips after it.
  template <int G>
  static __device__ __forceinline__ void syrk36_prefetch(const float* __restrict__ Hjj, int64_t ld, int valid, float4* hp,
                                                        int lane) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto ldb = [&](int u, int v) __attribute__((always_inline)) -> float4 {
      const int r = min(16 * u + (lane & 15), valid - 1);
      return *reinterpret_cast<const float4*>(Hjj + (int64_t)r * ld + 16 * v + 4 * (lane >> 4));
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) hp[v] = ldb(UH, v);
#pragma unroll
    for (int v = 0; v <= UL; ++v) hp[UH + 1 + v] = ldb(UL, v);
  }
  // tile(u, v) <- S = H (+ damping on the diagonal) - acc; rows / columns outside the matrix: identity
  template <int G>
  static __device__ __forceinline__ void syrk36_store(float* tile, const float4* hp, const f32x4* acc, int lane, int valid,
                                                      bool damp, float lam, int ellipsoidal, float eps) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto st = [&](int u, int v, const float4& h, const f32x4& a) __attribute__((always_inline)) {
      const int r = 16 * u + (lane & 15), c0 = 16 * v + 4 * (lane >> 4);
      float hv[4] = {h.x, h.y, h.z, h.w}, o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = c0 + k;
        float x = hv[k];
        if (u == v && r == c && damp) x = ellipsoidal ? x + (lam * x + eps) : x + lam;
        x -= a[k];
        if (r >= valid || c >= valid) x = (r == c) ? 1.f : 0.f;
        o[k] = x;
      }
      *reinterpret_cast<float4*>(tile + tblk<float>(u >> 1, v >> 1) + (r & 31) * 36 + (c0 & 31)) =
          make_float4(o[0], o[1], o[2], o[3]);
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) st(UH, v, hp[v], acc[v]);
#pragma unroll
    for (int v = 0; v <= UL; ++v) st(UL, v, hp[UH + 1 + v], acc[UH + 1 + v]);
  }
  // ---- 32x32 block helpers for the diagonal-tile factorisation (operands: sub-blocks of the LDS tile, row stride 36).
  //      Blk D[m][n]: a lane holds ONE row n = lane&31 of the block, register rho <-> column m = 8(rho>>2) + 4g + (rho&3)
  using Blk = f32x16;
  static __device__ __forceinline__ void blk_zero(Blk& d) {
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = 0.f;
  }
  static __device__ __forceinline__ void blk_sub(Blk& d, const Blk& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] -= a[i];
  }
  static __device__ __forceinline__ void blk_load(Blk& d, const float* blk, int lane) {
    const float* p = blk + (lane & 31) * 36 + 4 * (lane >> 5);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(p + 8 * q);
      d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w;
    }
  }
  static __device__ __forceinline__ void blk_store(const Blk& d, float* blk, int lane, float sign) {
    float* p = blk + (lane & 31) * 36 + 4 * (lane >> 5);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(p + 8 * q) =
          make_float4(sign * d[4 * q], sign * d[4 * q + 1], sign * d[4 * q + 2], sign * d[4 * q + 3]);
  }
  // D[m][n] += sum_k (asign * A[m][k]) * B[n][k]   (A, B: 32x32 blocks in LDS, rows m / n)
  static __device__ __forceinline__ void blk_mma(const float* Ablk, const float* Bblk, Blk& d, int lane, float asign) {
    const int o = (lane & 31) * 36 + 4 * (lane >> 5);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 fa = *reinterpret_cast<const float4*>(Ablk + o + 8 * q);
      const float4 fb = *reinterpret_cast<const float4*>(Bblk + o + 8 * q);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(asign * fa.x, fb.x, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(asign * fa.y, fb.y, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(asign * fa.z, fb.z, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(asign * fa.w, fb.w, d, 0, 0, 0);
    }
  }

  // ---- register-resident blocks (chol_potrf_kernel: the whole diagonal tile lives in ONE wave's registers) ----
  // D[m][n] += sum_k (asign * A[m][k]) * B[n][k] with A, B AND D in the C/D layout (lane = the block's own row, registers =
  // columns): an MFMA's k index is only a pairing of columns, and two blocks in this layout pair theirs identically
  // (register rho of lane group g <-> column 8(rho>>2) + 4g + (rho&3)).  No LDS, no data movement.
  static __device__ __forceinline__ void blk_mma_rr(const Blk& A, const Blk& B, Blk& d, float asign) {
#pragma unroll
    for (int i = 0; i < 16; ++i) d = __builtin_amdgcn_mfma_f32_32x32x2f32(asign * A[i], B[i], d, 0, 0, 0);
  }
  static __device__ __forceinline__ void blk_neg(Blk& d) {
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = -d[i];
  }
  // 32x32 block of a row-major global matrix -> registers; rows >= rv / columns >= cv (outside the matrix): identity on a
  // diagonal block, zero elsewhere
  static __device__ __forceinline__ void blk_load_global(Blk& d, const float* blk, const float* safe, int64_t ld, int rv, int cv,
                                                         bool diag, int lane) {
    const int r = lane & 31, g = lane >> 5;
    // (a sub-block wholly outside the matrix may lie outside the FRAME too: its lanes read ``safe`` -- 32 valid elements)
    const float* p = (r < rv ? blk + (int64_t)r * ld : safe) + 4 * g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(p + 8 * q);
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = 8 * q + 4 * g + k;
        d[4 * q + k] = (r < rv && c < cv) ? e[k] : ((diag && r == c) ? 1.f : 0.f);
      }
    }
  }
  // registers -> global (rows < rv only), scaled by sign
  static __device__ __forceinline__ void blk_store_global(const Blk& d, float* blk, int64_t ld, int rv, int lane, float sign) {
    const int r = lane & 31, g = lane >> 5;
    if (r < rv) {
      float* p = blk + (int64_t)r * ld + 4 * g;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(p + 8 * q) =
            make_float4(sign * d[4 * q], sign * d[4 * q + 1], sign * d[4 * q + 2], sign * d[4 * q + 3]);
    }
  }
  // rows of a 32-vector a lane is responsible for: NR of them, row blk_row(lane, i); the lanes with row_owner() write
  static constexpr int NR = 1;
  static __device__ __forceinline__ int blk_row(int lane, int) { return lane & 31; }
  static __device__ __forceinline__ bool row_owner(int lane) { return lane < 32; }
  // out[0] = sum_c X[row][c] * vec[c] for this lane's row (vec: 32 values in LDS); valid in every lane
  static __device__ __forceinline__ void blk_rowdot(const Blk& X, const float* vec, int lane, float (&out)[1]) {
    const int g = lane >> 5;
    // (explicit FMA chain: the function is inlined into two kernels whose results must agree bit for bit -- fwd_diag_block --
    //  and the compiler's contraction of a * b + c * d + ... depends on the surrounding code)
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4*>(vec + 8 * q + 4 * g);
      s = __builtin_fmaf(X[4 * q], v.x, s);
      s = __builtin_fmaf(X[4 * q + 1], v.y, s);
      s = __builtin_fmaf(X[4 * q + 2], v.z, s);
      s = __builtin_fmaf(X[4 * q + 3], v.w, s);
    }
    out[0] = s + __shfl_xor(s, 32);
  }
  // S = H (+ damping on the diagonal) - acc of the 36 lower 16x16 blocks -> the diagonal tile's place in the GLOBAL factor
  // (rows inside the matrix only; chol_potrf_kernel pads on load)
  template <int G>
  static __device__ __forceinline__ void syrk36_store_global(float* Lt, int64_t ld, const float4* hp, const f32x4* acc, int lane,
                                                             int valid, bool damp, float lam, int ellipsoidal, float eps) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto st = [&](int u, int v, const float4& h, const f32x4& a) __attribute__((always_inline)) {
      const int r = 16 * u + (lane & 15), c0 = 16 * v + 4 * (lane >> 4);
      if (r >= valid) return;
      float hv[4] = {h.x, h.y, h.z, h.w}, o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float x = hv[k];
        if (u == v && r == c0 + k && damp) x = ellipsoidal ? x + (lam * x + eps) : x + lam;
        o[k] = x - a[k];
      }
      *reinterpret_cast<float4*>(Lt + (int64_t)r * ld + c0) = make_float4(o[0], o[1], o[2], o[3]);
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) st(UH, v, hp[v], acc[v]);
#pragma unroll
    for (int v = 0; v <= UL; ++v) st(UL, v, hp[UH + 1 + v], acc[UH + 1 + v]);
  }
};

template <>
struct Engine<double> {
  struct Acc {
    f64x4 v[2][8];
  };
  static __device__ __forceinline__ void zero(Acc& a) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) a.v[h][i][j] = 0.0;
  }
  static __device__ __forceinline__ void chunk(const double* sA, const double* sBw, Acc& acc, int lane) {
    const int rl = lane & 15, kq = lane >> 4;
    constexpr int LDT = CT<double>::LDT;
#pragma unroll
    for (int ks = 0; ks < CT<double>::KB / 8; ++ks) {
      double2 fb[2];
      fb[0] = *reinterpret_cast<const double2*>(sBw + rl * LDT + 8 * ks + 2 * kq);
      fb[1] = *reinterpret_cast<const double2*>(sBw + (16 + rl) * LDT + 8 * ks + 2 * kq);
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        const double2 fa = *reinterpret_cast<const double2*>(sA + (16 * cb + rl) * LDT + 8 * ks + 2 * kq);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          acc.v[h][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.x, fb[h].x, acc.v[h][cb], 0, 0, 0);
          acc.v[h][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa.y, fb[h].y, acc.v[h][cb], 0, 0, 0);
        }
      }
    }
  }

  // ---- 32x32 block helpers (see Engine<float>): Blk.v[mh][nh][rho] <-> row n = 16nh + (lane&15),
  //      column m = 16mh + (lane>>4) + 4rho; LDS row stride 34
  struct Blk {
    f64x4 v[2][2];
  };
  // see Engine<float>::syrk36; staged rows have stride 20 doubles (40 words), a k-chunk is 16 wide, lane (r, kq) reads
  // doubles 2kq, 2kq+1 and 8+2kq, 9+2kq (words 4kq and 16+4kq): conflict free
  static constexpr int SYRK_LDT = 20;
  // (a 32-column k-chunk would be staged as TWO 16-wide sub-chunks of 128 x SYRK_LDT -- kloop_f's SPLIT16 layout -- so that each
  //  keeps the conflict-free stride; syrk36 runs once per sub-chunk)
  static constexpr int SYRK_SUBS = CT<double>::KB / 16;
  static constexpr int SYRK_STAGE = SYRK_SUBS * 128 * SYRK_LDT;
  using Sy = f64x4;
  template <int G>
  static __device__ __forceinline__ void syrk36(const double* sA, f64x4* acc, int lane) {
#pragma unroll
    for (int h = 0; h < SYRK_SUBS; ++h) syrk36_sub<G>(sA + h * 128 * SYRK_LDT, acc, lane);
  }
  template <int G>
  static __device__ __forceinline__ void syrk36_sub(const double* sA, f64x4* acc, int lane) {
    constexpr int UH = 4 + G, UL = 3 - G;
    const int o = (lane & 15) * 20 + 2 * (lane >> 4);
    double fbh[4], fbl[4];
    {
      const double2 a = *reinterpret_cast<const double2*>(sA + 16 * UH * 20 + o), b = *reinterpret_cast<const double2*>(sA + 16 * UH * 20 + o + 8);
      const double2 c = *reinterpret_cast<const double2*>(sA + 16 * UL * 20 + o), d = *reinterpret_cast<const double2*>(sA + 16 * UL * 20 + o + 8);
      fbh[0] = a.x; fbh[1] = a.y; fbh[2] = b.x; fbh[3] = b.y;
      fbl[0] = c.x; fbl[1] = c.y; fbl[2] = d.x; fbl[3] = d.y;
    }
#pragma unroll
    for (int v = 0; v <= UH; ++v) {
      double fa[4];
      if (v == UH) {
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[m] = fbh[m];
      } else if (v == UL) {
#pragma unroll
        for (int m = 0; m < 4; ++m) fa[m] = fbl[m];
      } else {
        const double2 a = *reinterpret_cast<const double2*>(sA + 16 * v * 20 + o), b = *reinterpret_cast<const double2*>(sA + 16 * v * 20 + o + 8);
        fa[0] = a.x; fa[1] = a.y; fa[2] = b.x; fa[3] = b.y;
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) acc[v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[m], fbh[m], acc[v], 0, 0, 0);
      if (v <= UL) {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[UH + 1 + v] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[m], fbl[m], acc[UH + 1 + v], 0, 0, 0);
      }
    }
  }
  // H_jj blocks global -> registers before the K-loop / S = H (+ damping) - acc -> LDS afterwards (see Engine<float>)
  template <int G>
  static __device__ __forceinline__ void syrk36_prefetch(const double* __restrict__ Hjj, int64_t ld, int valid, f64x4* hp,
                                                        int lane) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto ldb = [&](int u, int v) __attribute__((always_inline)) -> f64x4 {
      const double* p = Hjj + (int64_t)min(16 * u + (lane & 15), valid - 1) * ld + 16 * v + (lane >> 4);
      f64x4 h;
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) h[rho] = p[4 * rho];
      return h;
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) hp[v] = ldb(UH, v);
#pragma unroll
    for (int v = 0; v <= UL; ++v) hp[UH + 1 + v] = ldb(UL, v);
  }
  template <int G>
  static __device__ __forceinline__ void syrk36_store(double* tile, const f64x4* hp, const f64x4* acc, int lane, int valid,
                                                      bool damp, double lam, int ellipsoidal, double eps) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto st = [&](int u, int v, const f64x4& h, const f64x4& a) __attribute__((always_inline)) {
      const int r = 16 * u + (lane & 15), c0 = 16 * v + (lane >> 4);
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const int c = c0 + 4 * rho;
        double x = h[rho];
        if (u == v && r == c && damp) x = ellipsoidal ? x + (lam * x + eps) : x + lam;
        x -= a[rho];
        if (r >= valid || c >= valid) x = (r == c) ? 1.0 : 0.0;
        tile[tblk<double>(u >> 1, v >> 1) + (r & 31) * 34 + (c & 31)] = x;
      }
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) st(UH, v, hp[v], acc[v]);
#pragma unroll
    for (int v = 0; v <= UL; ++v) st(UL, v, hp[UH + 1 + v], acc[UH + 1 + v]);
  }
  static __device__ __forceinline__ void blk_zero(Blk& d) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) d.v[a][b][i] = 0.0;
  }
  static __device__ __forceinline__ void blk_sub(Blk& d, const Blk& a) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) d.v[p][q][i] -= a.v[p][q][i];
  }
  static __device__ __forceinline__ void blk_load(Blk& d, const double* blk, int lane) {
    const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) d.v[mh][nh][rho] = blk[(16 * nh + rl) * 34 + 16 * mh + kq + 4 * rho];
  }
  static __device__ __forceinline__ void blk_store(const Blk& d, double* blk, int lane, double sign) {
    const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
      for (int nh = 0; nh < 2; ++nh)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) blk[(16 * nh + rl) * 34 + 16 * mh + kq + 4 * rho] = sign * d.v[mh][nh][rho];
  }
  static __device__ __forceinline__ void blk_mma(const double* Ablk, const double* Bblk, Blk& d, int lane, double asign) {
    const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const double a0 = asign * Ablk[rl * 34 + 4 * kk + kq], a1 = asign * Ablk[(16 + rl) * 34 + 4 * kk + kq];
      const double b0 = Bblk[rl * 34 + 4 * kk + kq], b1 = Bblk[(16 + rl) * 34 + 4 * kk + kq];
      d.v[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, d.v[0][0], 0, 0, 0);
      d.v[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, d.v[0][1], 0, 0, 0);
      d.v[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, d.v[1][0], 0, 0, 0);
      d.v[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d.v[1][1], 0, 0, 0);
    }
  }

  // ---- register-resident blocks (see Engine<float>): Blk.v[kh][rowhalf][rho] = X[16 rowhalf + (lane&15)][16 kh + (lane>>4) + 4 rho],
  //      so MFMA (kh, rho) contracts the four consecutive columns 16 kh + 4 rho + {0..3} of both operands ----
  static __device__ __forceinline__ void blk_mma_rr(const Blk& A, const Blk& B, Blk& d, double asign) {
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const double a0 = asign * A.v[kh][0][rho], a1 = asign * A.v[kh][1][rho];
        const double b0 = B.v[kh][0][rho], b1 = B.v[kh][1][rho];
        d.v[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, d.v[0][0], 0, 0, 0);
        d.v[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, d.v[0][1], 0, 0, 0);
        d.v[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, d.v[1][0], 0, 0, 0);
        d.v[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d.v[1][1], 0, 0, 0);
      }
  }
  static __device__ __forceinline__ void blk_neg(Blk& d) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) d.v[a][b][i] = -d.v[a][b][i];
  }
  static __device__ __forceinline__ void blk_load_global(Blk& d, const double* blk, const double* safe, int64_t ld, int rv, int cv,
                                                         bool diag, int lane) {
    const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      const int r = 16 * nh + rl;
      const double* p = (r < rv ? blk + (int64_t)r * ld : safe) + kq;
#pragma unroll
      for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) {
          const int c = 16 * mh + kq + 4 * rho;
          const double x = p[16 * mh + 4 * rho];
          d.v[mh][nh][rho] = (r < rv && c < cv) ? x : ((diag && r == c) ? 1.0 : 0.0);
        }
    }
  }
  static __device__ __forceinline__ void blk_store_global(const Blk& d, double* blk, int64_t ld, int rv, int lane, double sign) {
    const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      const int r = 16 * nh + rl;
      if (r < rv) {
        double* p = blk + (int64_t)r * ld + kq;
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
          for (int rho = 0; rho < 4; ++rho) p[16 * mh + 4 * rho] = sign * d.v[mh][nh][rho];
      }
    }
  }
  static constexpr int NR = 2;
  static __device__ __forceinline__ int blk_row(int lane, int i) { return 16 * i + (lane & 15); }
  static __device__ __forceinline__ bool row_owner(int lane) { return lane < 16; }
  static __device__ __forceinline__ void blk_rowdot(const Blk& X, const double* vec, int lane, double (&out)[2]) {
    const int kq = lane >> 4;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      double s = 0.0;
#pragma unroll
      for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int rho = 0; rho < 4; ++rho) s = __builtin_fma(X.v[mh][nh][rho], vec[16 * mh + kq + 4 * rho], s);
      s += __shfl_xor(s, 16);
      out[nh] = s + __shfl_xor(s, 32);
    }
  }
  template <int G>
  static __device__ __forceinline__ void syrk36_store_global(double* Lt, int64_t ld, const f64x4* hp, const f64x4* acc, int lane,
                                                             int valid, bool damp, double lam, int ellipsoidal, double eps) {
    constexpr int UH = 4 + G, UL = 3 - G;
    auto st = [&](int u, int v, const f64x4& h, const f64x4& a) __attribute__((always_inline)) {
      const int r = 16 * u + (lane & 15), c0 = 16 * v + (lane >> 4);
      if (r >= valid) return;
#pragma unroll
      for (int rho = 0; rho < 4; ++rho) {
        const int c = c0 + 4 * rho;
        double x = h[rho];
        if (u == v && r == c && damp) x = ellipsoidal ? x + (lam * x + eps) : x + lam;
        Lt[(int64_t)r * ld + c] = x - a[rho];
      }
    };
#pragma unroll
    for (int v = 0; v <= UH; ++v) st(UH, v, hp[v], acc[v]);
#pragma unroll
    for (int v = 0; v <= UL; ++v) st(UL, v, hp[UH + 1 + v], acc[UH + 1 + v]);
  }
};

// Optional rider on the SYRK K-loop of chol_diag: the panel rows L_j,0:j pass through LDS anyway, so
// t[r] = sum_k L[row0+r][k] y[k] (the forward-substitution update) costs 16 VALU FMAs per thread and
// chunk in the shadow of the MFMAs.  Thread pair (2r, 2r+1) splits the chunk's k range in two.
struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// ``after_issue`` runs right after the loads of the first k-chunk(s) have been ISSUED: whatever else a kernel wants in
// flight before its K-loop (H tile, solve panel) goes there, so that its latency overlaps the first chunk's instead of
// preceding it.
//
// ``ktiles`` (tile-sparse factorisation, thx_chol_factor_sparse): instead of the contiguous range [0, K) the loop visits the
// TILE-wide column blocks ktiles[0 .. K / TILE) -- the block columns in which BOTH operand row panels are structurally
// non-zero.  The list is wave uniform (scalar loads); skipping a block of exact zeros leaves every accumulator bit unchanged.
// SPLIT16 (fp64 SYRK): the chunk's columns [16 h, 16 h + 16) are staged as sub-chunk h at sA + h * 128 * LDT, row stride LDT.
// ``ksa`` / ``ksb`` (tile-packed factor): per K-list element the SLOT of the A / B operand tile; Arows / Brows then point at the
// problem's packed buffer, ``ld`` is TILE and ``packed_elems`` the buffer's extent (rows of a tile beyond the matrix are zero in
// the buffer itself, never written).
template <typename T, bool SAME, bool GEMV, int LDT, bool SPLIT16 = false, int NT = 256, int AHEAD_OVR = 0, int BROWS = TILE,
          typename Compute, typename Hook = NoHook>
__device__ __forceinline__ void kloop_f(const T* __restrict__ Arows, int validA, const T* __restrict__ Brows,
                                        int validB, int64_t ld, int K, T* sA, T* sB, int tid, const T* gemv_y,
                                        T* gemv_part, Compute&& compute, Hook&& after_issue = NoHook{},
                                        const int32_t* __restrict__ ktiles = nullptr, const int32_t* __restrict__ ksa = nullptr,
                                        const int32_t* __restrict__ ksb = nullptr, int64_t packed_elems = 0,
                                        bool gemv_compact = false) {
  // (gemv_compact: gemv_y holds the K-LIST's blocks of y back to back -- element kc * KB belongs to chunk kc -- instead of the
  //  whole vector: the level schedule's diagonal kernels, whose K-lists are short and scattered over all of y)
  using C = CT<T>;
  using V = typename C::V;
  constexpr int TPR = C::KB / C::VEC;   // threads per staged row (16 bytes each)
  static_assert(!GEMV || NT == 256, "the fused GEMV pairs the 256 threads with the 128 rows");
  constexpr int RPP = NT / TPR;         // rows per pass of the NT (256; the 8-wave fp64 off-diagonal kernel: 512) threads
  constexpr int NP = TILE / RPP;        // passes: fp32 4 x 32 rows, fp64 8 x 16 rows
  constexpr int NPB = BROWS / RPP;      // (operand B of the fp64 half-tile kernel: 64 rows -- the other passes are neither loaded nor staged)
  static_assert(BROWS % RPP == 0 && NPB >= 1 && NPB <= NP, "B rows: whole passes");
  const int lrow = tid / TPR, lc = tid % TPR;
  // element offset of this thread's 16-byte piece inside a staged row (set)
  const int scol = SPLIT16 ? ((lc * C::VEC) >> 4) * 128 * LDT + ((lc * C::VEC) & 15) : lc * C::VEC;
  // Operand rows through BUFFER loads: base pointer + extent live in a 4-SGPR resource, each lane contributes a 32-bit
  // byte offset, the k-chunk offset is a scalar -- no 64-bit per-row addresses in VGPRs (the fp64 kernels, two
  // workgroups per CU = 256 VGPRs, spilled them, and every reload put an s_waitcnt vmcnt(0) into the prefetch), and rows
  // outside the matrix are zeroed by the hardware bounds check (extent = valid rows) instead of v_cndmask / exec branches.
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  const bool packed = ksa != nullptr;
  const int extA = packed ? (int)(packed_elems * (int64_t)sizeof(T)) : (int)((int64_t)validA * ld * (int64_t)sizeof(T));
  const int extB = packed ? extA : (int)((int64_t)(SAME ? validA : validB) * ld * (int64_t)sizeof(T));
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(Arows), 0, extA, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(SAME ? Arows : Brows), 0, extB, 0x00020000);
  unsigned voff[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) voff[u] = (unsigned)(((lrow + RPP * u) * (int)ld + lc * C::VEC) * (int)sizeof(T));
  // Register prefetch, AHEAD k-chunks deep: 128 bytes per staged row in flight.  fp32: one 32-column chunk (a second register
  // set measured no gain: 47.3-47.7 ms either way); fp64: two 16-column chunks -- a 16-column chunk is half the MFMA time of an
  // fp32 one, one chunk ahead does not cover the load latency (factor -2.9 %).
  constexpr int AHEAD = AHEAD_OVR ? AHEAD_OVR : (C::KB * (int)sizeof(T) <= 128 ? 2 : 1);   // (AHEAD_OVR: the fp64 half-tile kernel, 128 VGPRs)
  uint4 ra[AHEAD][NP], rb[AHEAD][NP];
  // (so.x / so.y: scalar byte offsets of the chunk inside the A / B operand buffers; the same unless the factor is tile-packed)
  auto gload = [&](uint4 (&xa)[NP], uint4 (&xb)[NP], int2 so) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const u32x4 va = __builtin_amdgcn_raw_buffer_load_b128(rsA, voff[u], so.x, 0);
      xa[u] = make_uint4(va.x, va.y, va.z, va.w);
      if (!SAME && u < NPB) {
        const u32x4 vb = __builtin_amdgcn_raw_buffer_load_b128(rsB, voff[u], so.y, 0);
        xb[u] = make_uint4(vb.x, vb.y, vb.z, vb.w);
      }
    }
  };
  const int nk = K / C::KB;
  constexpr int CPT = TILE / C::KB;   // k-chunks per tile
  // first column of k-chunk kc
  // (the list is read through the constant address space: a SCALAR load.  As a plain global load the compiler issued a vector
  // load + s_waitcnt vmcnt(0) in front of every chunk's prefetch and wrapped each buffer load in a waterfall loop, since it
  // could not prove the offset wave uniform.)
  typedef const int32_t __attribute__((address_space(4))) * klist_t;
  const klist_t kl = (klist_t)(uintptr_t)ktiles;
  const klist_t ka = (klist_t)(uintptr_t)ksa, kb = (klist_t)(uintptr_t)ksb;
  auto kof = [&](int kc) __attribute__((always_inline)) -> int {
    const int k0 = kl ? kl[kc / CPT] * TILE + (kc % CPT) * C::KB : kc * C::KB;
    return __builtin_amdgcn_readfirstlane(k0);
  };
  // byte offsets of chunk kc in the two operand buffers
  auto sof = [&](int kc) __attribute__((always_inline)) -> int2 {
    if (!packed) {
      const int so = kof(kc) * (int)sizeof(T);
      return make_int2(so, so);
    }
    const int within = (kc % CPT) * C::KB;
    const int a = (ka[kc / CPT] * TILE * TILE + within) * (int)sizeof(T);
    const int bq = SAME ? a : (kb[kc / CPT] * TILE * TILE + within) * (int)sizeof(T);
    return make_int2(__builtin_amdgcn_readfirstlane(a), __builtin_amdgcn_readfirstlane(bq));
  };
  T gsum = T(0);
  // one k-chunk: registers -> LDS, refill the registers with the chunk AHEAD steps on, MFMAs on the staged chunk
  // (a static s_setprio per hardware wave slot, to push the two co-resident workgroups out of lockstep, measured no gain)
  auto step = [&](uint4 (&xa)[NP], uint4 (&xb)[NP], int kc) __attribute__((always_inline)) {
    // column of the chunk to prefetch: the K-list entry is fetched here so that its (scalar) load completes under the staging
    const int2 knext = kc + AHEAD < nk ? sof(kc + AHEAD) : make_int2(0, 0);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      const int row = lrow + RPP * u;
      *reinterpret_cast<uint4*>(sA + row * LDT + scol) = xa[u];
      if (!SAME && u < NPB) *reinterpret_cast<uint4*>(sB + row * LDT + scol) = xb[u];
    }
    __syncthreads();
    if (kc + AHEAD < nk) gload(xa, xb, knext);
    if constexpr (GEMV) {
      if (gemv_y) {
        constexpr int HALF = C::KB / 2;
        // (thread pair (2r, 2r+1): the two 16-column halves of row r -- with SPLIT16 the two sub-chunks)
        const V* rp = reinterpret_cast<const V*>(sA + (tid >> 1) * LDT + (SPLIT16 ? (tid & 1) * 128 * LDT : (tid & 1) * HALF));
        const V* yp = reinterpret_cast<const V*>(gemv_y + (gemv_compact ? kc * C::KB : kof(kc)) + (tid & 1) * HALF);
#pragma unroll
        for (int i = 0; i < HALF / C::VEC; ++i) {
          const V a = rp[i], yv = yp[i];
          if constexpr (sizeof(T) == 4) {
            gsum += a.x * yv.x; gsum += a.y * yv.y; gsum += a.z * yv.z; gsum += a.w * yv.w;
          } else {
            gsum += a.x * yv.x; gsum += a.y * yv.y;
          }
        }
      }
    }
    compute();  // MFMAs on the staged chunk (sA / sB)
  };
#pragma unroll
  for (int a = 0; a < AHEAD; ++a)
    if (a < nk) gload(ra[a], rb[a], sof(a));
  after_issue();
  for (int kc = 0; kc < nk; kc += AHEAD) {
    step(ra[0], rb[0], kc);
    if constexpr (AHEAD == 2) {
      if (kc + 1 < nk) step(ra[1], rb[1], kc + 1);
    }
  }
  if constexpr (GEMV) {
    if (gemv_part) *gemv_part = gsum;
  }
}

template <typename T, bool SAME, bool GEMV = false, typename Hook = NoHook>
__device__ __forceinline__ void kloop(const T* __restrict__ Arows, int validA, const T* __restrict__ Brows,
                                      int validB, int64_t ld, int K, T* sA, T* sB,
                                      typename Engine<T>::Acc& acc, int tid, const T* gemv_y = nullptr,
                                      T* gemv_part = nullptr, Hook&& after_issue = NoHook{},
                                      const int32_t* __restrict__ ktiles = nullptr, const int32_t* __restrict__ ksa = nullptr,
                                      const int32_t* __restrict__ ksb = nullptr, int64_t packed_elems = 0) {
  const int wave = tid >> 6, lane = tid & 63;
  kloop_f<T, SAME, GEMV, CT<T>::LDT>(Arows, validA, Brows, validB, ld, K, sA, sB, tid, gemv_y, gemv_part, [&]() __attribute__((always_inline)) {
    Engine<T>::chunk(sA, (SAME ? sA : sB) + 32 * wave * CT<T>::LDT, acc, lane);
  }, after_issue, ktiles, ksa, ksb, packed_elems);
}

}  // namespace thx
