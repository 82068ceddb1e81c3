#pragma once
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_potrf.cuh"

namespace thx {

// ------------------------------------------------------------------------------------------------
// triangular solves with one right-hand side per problem, one workgroup per problem, HBM bound
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ void panel_g2l(const T* __restrict__ Pn, T* tile, int tid) {
  using C = CT<T>;
  constexpr int CPR = TILE / C::VEC, RPP = 256 / CPR;
  const int c = (tid % CPR) * C::VEC;
#pragma unroll 4
  for (int rr = tid / CPR; rr < TILE; rr += RPP)
    *reinterpret_cast<uint4*>(tile + rr * C::LDM + c) = *reinterpret_cast<const uint4*>(Pn + rr * TILE + c);
}

// The substitutions read the ten 32x32 sub-blocks on and below the panel's diagonal only (panel_forward: row block s, columns
// [0, 32 s + 32); panel_backward: column block t, rows [32 t, 128)): this copy leaves the six upper ones out -- their part of the LDS
// tile stays unwritten and unread, the layout is panel_g2l's.
// Sub-block by sub-block, every thread one (fp64: two) 16-byte group of each: no predicate, so the ten (twenty) loads are independent
// and in flight together, where panel_g2l's row loop goes to memory four times (eight) per panel.
template <typename T>
__device__ __forceinline__ void panel_g2l_lower(const T* __restrict__ Pn, T* tile, int tid) {
  using C = CT<T>;
  constexpr int GPS = 32 / C::VEC, IPS = 32 * GPS / 256;   // 16-byte groups per sub-block row; groups per thread and sub-block
  static_assert(IPS * 256 == 32 * GPS, "a sub-block is a whole number of rounds of the workgroup");
  uint4 v[10 * IPS];
#pragma unroll
  for (int sb = 0; sb < 10; ++sb) {
    const int sr = sb < 1 ? 0 : sb < 3 ? 1 : sb < 6 ? 2 : 3, sc = sb - sr * (sr + 1) / 2;   // (sub-block row, column), sc <= sr
#pragma unroll
    for (int i = 0; i < IPS; ++i) {
      const int it = tid + 256 * i, r = 32 * sr + it / GPS, c = 32 * sc + (it % GPS) * C::VEC;
      v[IPS * sb + i] = *reinterpret_cast<const uint4*>(Pn + r * TILE + c);
    }
  }
#pragma unroll
  for (int sb = 0; sb < 10; ++sb) {
    const int sr = sb < 1 ? 0 : sb < 3 ? 1 : sb < 6 ? 2 : 3, sc = sb - sr * (sr + 1) / 2;
#pragma unroll
    for (int i = 0; i < IPS; ++i) {
      const int it = tid + 256 * i, r = 32 * sr + it / GPS, c = 32 * sc + (it % GPS) * C::VEC;
      *reinterpret_cast<uint4*>(tile + r * C::LDM + c) = v[IPS * sb + i];
    }
  }
}

// (env: the envelope path of the dense-frame kernels keeps the 128 first-column values of the current block row behind ubuf)
template <typename T>
static size_t solve_smem(int npad, bool env = false) {
  return (size_t)128 * CT<T>::LDM * sizeof(T) + (size_t)(npad + 128 + 32) * sizeof(T) + (env ? 128 * sizeof(int32_t) : 0);
}

// Row-wise tile pattern of L for the list-driven solves (thx_chol_solve_sparse): for block row i the column tiles j < i with
// L_ij structurally non-zero.  Null pointers = dense.
struct RowPat {
  const int32_t* __restrict__ row_ptr;   // [ntiles + 1]
  const int32_t* __restrict__ row_tile;  // [row_ptr[ntiles]]
  const int32_t* __restrict__ row_slot;  // tile-packed factor: the slot of every listed tile (else nullptr)
  int32_t nslots;                        // tile-packed factor: slots per problem (else 0)
  // LEVEL schedule (thx_chol_solve_levels): one launch = the block rows [j0, j0 + gridDim.y) of one elimination-tree level (they do
  // not depend on each other), one workgroup per (problem, block row); j0 < 0: one workgroup walks all block rows of its problem
  int32_t j0;
  const int32_t* __restrict__ tile_valid;   // per-tile padding (see TilePat)
};

// L y = rhs (stand-alone; the LM iteration gets y from the factorisation).
// LIST = false: the whole solution vector lives in LDS (n <= ~23 k fp32 / 3.4 k fp64) and every tile of a block row is streamed.
// LIST = true : the tiles of the row's list only, and the vector stays in global memory (L2) -- no limit on n.
// ENV (dense frame only): row r of L holds exact zeros left of row_first[r] (thx_chol_solve_env).  For a VEC group that lies wholly
// left of it a lane re-reads the row's first needed group (no new bytes from HBM; unconditional loads, see chol_bwd_kernel) and adds
// 0 instead of the group's dot product, which is a sum of exact zeros: each lane's partial sums keep their order and their bits.
template <typename T, bool LIST, bool ENV = false>
__global__ void __launch_bounds__(256)
chol_fwd_kernel(const T* __restrict__ L, const T* __restrict__ panel, const T* __restrict__ rhs, T* __restrict__ y,
                int n, int64_t ld, int64_t ldv, int ntiles, RowPat rp, const int32_t* __restrict__ row_first) {
  static_assert(!(LIST && ENV), "the envelope path is the dense frame's");
  using C = CT<T>;
  using V = typename C::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const int npad = LIST ? 0 : ntiles * TILE;
  T* yv = tile + 128 * C::LDM;  // [npad]
  T* tv = yv + npad;            // [128]
  T* ubuf = tv + 128;           // [32]
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool packed = LIST && rp.nslots > 0;
  const T* Lb = L + (int64_t)b * (packed ? (int64_t)rp.nslots * TILE * TILE : ld * ld);
  const T* rb = rhs + (int64_t)b * ldv;
  T* yb = y + (int64_t)b * ldv;
  if constexpr (!LIST) {
    for (int k = tid; k < npad; k += 256) yv[k] = k < n ? rb[k] : T(0);
    __syncthreads();
  }
  constexpr int QPT = TILE / C::VEC;   // VEC-wide column groups per tile
  const int jlo = (LIST && rp.j0 >= 0) ? rp.j0 + (int)blockIdx.y : 0, jhi = (LIST && rp.j0 >= 0) ? jlo + 1 : ntiles;
  for (int jb = jlo; jb < jhi; ++jb) {
    const int row0 = jb * TILE, valid = (LIST && rp.tile_valid) ? rp.tile_valid[jb] : min(TILE, n - row0);
    if constexpr (LIST) panel_g2l<T>(panel + ((int64_t)b * ntiles + jb) * TILE * TILE, tile, tid);
    else panel_g2l_lower<T>(panel + ((int64_t)b * ntiles + jb) * TILE * TILE, tile, tid);
    // t[r] = sum_{k < row0} L[row0 + r][k] y[k]: wave w takes rows r = w (mod 4), four rows in flight
    const int l0 = LIST ? rp.row_ptr[jb] : 0;
    const int items = LIST ? (rp.row_ptr[jb + 1] - l0) * QPT : row0 / C::VEC;
    for (int rr = wave; rr < TILE; rr += 16) {
      T s[4] = {T(0), T(0), T(0), T(0)};
      int fr[4] = {0, 0, 0, 0};   // ENV: first 16-byte group of the wave's four rows, as chol_bwd_kernel's fb (wave uniform)
      if constexpr (ENV) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (rr + 4 * u < valid) fr[u] = min(row_first[row0 + rr + 4 * u] / C::VEC * C::VEC, row0 - C::VEC);
      }
      for (int it = lane; it < items; it += 64) {
        const int k = LIST ? rp.row_tile[l0 + it / QPT] * TILE + (it % QPT) * C::VEC : it * C::VEC;
        // the listed tile's rows: dense frame (row0 + r) * ld + k, or the packed tile's own 128 x 128 block
        const T* Lt_ = packed ? Lb + (int64_t)rp.row_slot[l0 + it / QPT] * TILE * TILE + (it % QPT) * C::VEC : Lb + (int64_t)row0 * ld + k;
        const int64_t lds_ = packed ? TILE : ld;
        V yk;
        if constexpr (LIST) {   // (scalar loads: a row of the vector need not be 16-byte aligned)
          if constexpr (sizeof(T) == 4) yk = V{yb[k], yb[k + 1], yb[k + 2], yb[k + 3]};
          else yk = V{yb[k], yb[k + 1]};
        } else {
          yk = *reinterpret_cast<const V*>(yv + k);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = rr + 4 * u;
          if (r < valid) {
            const int out = ENV ? max(fr[u] - k, 0) : 0;   // > 0: left of the row's envelope -- re-read its first group, add 0
            const V lv = *reinterpret_cast<const V*>(Lt_ + (int64_t)r * lds_ + out);
            T d;
            if constexpr (sizeof(T) == 4) d = lv.x * yk.x + lv.y * yk.y + lv.z * yk.z + lv.w * yk.w;
            else d = lv.x * yk.x + lv.y * yk.y;
            s[u] += out > 0 ? T(0) : d;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const T t = wave_sum(s[u]);
        if (lane == 0) tv[rr + 4 * u] = t;
      }
    }
    __syncthreads();
    if (tid < TILE) {
      if constexpr (LIST) tv[tid] = (tid < valid ? rb[row0 + tid] : T(0)) - tv[tid];
      else tv[tid] = yv[row0 + tid] - tv[tid];
    }
    __syncthreads();
    if (wave == 0) panel_forward<T>(tile, tv, ubuf, lane);
    __syncthreads();
    if (tid < TILE) {
      if constexpr (LIST) {
        if (tid < valid) yb[row0 + tid] = tv[tid];
      } else {
        yv[row0 + tid] = tv[tid];
      }
    }
    __syncthreads();   // (LIST: also makes the block of y visible to the whole workgroup before the next row reads it)
  }
  if constexpr (!LIST)
    for (int k = tid; k < n; k += 256) yb[k] = yv[k];
}

// L^T x = y : right-looking from the last block row; every (LIST: every structurally non-zero) tile of L is streamed once
// ENV (dense frame only): row r of L holds exact zeros left of row_first[r] (thx_chol_solve_backward_env).  The push keeps its rows
// (uniform across the workgroup, unrolled by 8) and the order of its fused multiply-adds.  A thread that owns columns k .. k + VEC - 1
// needs row r only when k + VEC > row_first[r]; otherwise it re-reads the row's FIRST needed 16-byte group (which the thread that
// owns it fetches anyway: no new bytes from HBM) and multiplies by 0 instead of x_r.  The loads stay unconditional on purpose: with
// each of the eight loads under its own lane predicate the compiler waits for vmcnt(0) in front of every one of them, and the
// kernel took 6.80 ms instead of 3.45 at the headline size.  What changes is a product with an exact zero turned into a product of
// a finite number with zero, so x is bit-identical for info == 0.  A factor that failed (info != 0) may hold non-finite values, and
// 0 * inf is NaN on either path, in other places: such a solution is garbage either way.
template <typename T, bool LIST, bool ENV = false>
__global__ void __launch_bounds__(256)
chol_bwd_kernel(const T* __restrict__ L, const T* __restrict__ panel, const T* __restrict__ yin, T* __restrict__ x,
                int n, int64_t ld, int64_t ldv, int ntiles, RowPat rp, const int32_t* __restrict__ row_first) {
  static_assert(!(LIST && ENV), "the envelope path is the dense frame's");
  using C = CT<T>;
  using V = typename C::V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  const int npad = LIST ? 0 : ntiles * TILE;
  T* z = tile + 128 * C::LDM;  // [npad]
  T* xb = z + npad;            // [128] current block
  T* ubuf = xb + 128;          // [32]
  int32_t* fb = reinterpret_cast<int32_t*>(ubuf + 32);   // ENV: [128] first needed 16-byte group of the current block's rows
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool packed = LIST && rp.nslots > 0;
  const T* Lb = L + (int64_t)b * (packed ? (int64_t)rp.nslots * TILE * TILE : ld * ld);
  T* zg = x + (int64_t)b * ldv;   // LIST: the working vector IS the output (global, L2 resident)
  if constexpr (LIST) {
    if (yin != x && rp.j0 < 0)   // (level schedule: the host copies y into x before the first level's launch)
      for (int k = tid; k < n; k += 256) zg[k] = yin[(int64_t)b * ldv + k];
  } else {
    for (int k = tid; k < npad; k += 256) z[k] = k < n ? yin[(int64_t)b * ldv + k] : T(0);
  }
  __syncthreads();
  constexpr int QPT = TILE / C::VEC;
  // (level schedule: the rows of a level scatter into DISJOINT column blocks of z -- the non-zero rows of a block column are a
  //  chain of the elimination tree, no two of them on one level -- so the push needs no atomics)
  const int jhi = (LIST && rp.j0 >= 0) ? rp.j0 + (int)blockIdx.y : ntiles - 1, jlo = (LIST && rp.j0 >= 0) ? jhi : 0;
  for (int jb = jhi; jb >= jlo; --jb) {
    const int row0 = jb * TILE, valid = (LIST && rp.tile_valid) ? rp.tile_valid[jb] : min(TILE, n - row0);
    if constexpr (LIST) panel_g2l<T>(panel + ((int64_t)b * ntiles + jb) * TILE * TILE, tile, tid);
    else panel_g2l_lower<T>(panel + ((int64_t)b * ntiles + jb) * TILE * TILE, tile, tid);
    if (tid < TILE) xb[tid] = LIST ? (tid < valid ? zg[row0 + tid] : T(0)) : z[row0 + tid];
    if constexpr (ENV) {
      // the row's first 16-byte group; a row that begins inside the diagonal tile keeps the last group in front of it (zeros)
      if (tid < TILE) fb[tid] = tid < valid ? min(row_first[row0 + tid] / C::VEC * C::VEC, row0 - C::VEC) : 0;
    }
    __syncthreads();
    if (wave == 0) panel_backward<T>(tile, xb, ubuf, lane);
    __syncthreads();
    if (tid < TILE) {
      if constexpr (LIST) {
        if (tid < valid) zg[row0 + tid] = xb[tid];
      } else {
        z[row0 + tid] = xb[tid];
      }
    }
    // z[0:row0] -= L[row0 : row0 + valid, 0:row0]^T x_block : a thread owns VEC consecutive columns,
    // rows unrolled by 8 (independent 16-byte loads in flight), x broadcast from LDS
    const int l0 = LIST ? rp.row_ptr[jb] : 0;
    const int items = LIST ? (rp.row_ptr[jb + 1] - l0) * QPT : row0 / C::VEC;
    for (int it = tid; it < items; it += 256) {
      const int k = LIST ? rp.row_tile[l0 + it / QPT] * TILE + (it % QPT) * C::VEC : it * C::VEC;
      T s[4] = {T(0), T(0), T(0), T(0)};
      const T* Lk = packed ? Lb + (int64_t)rp.row_slot[l0 + it / QPT] * TILE * TILE + (it % QPT) * C::VEC : Lb + (int64_t)row0 * ld + k;
      const int64_t lds_ = packed ? (int64_t)TILE : ld;   // (row stride of the listed tile)
      // eight rows r0 .. r0 + 7: the loads (out: ENV, how far left of the row's first 16-byte group the thread's columns lie; 0 =
      // inside the envelope), and their multiply-adds in row order
      auto load8 = [&](V (&lv)[8], int (&out)[8], int r0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          out[u] = ENV ? max(fb[r0 + u] - k, 0) : 0;
          lv[u] = *reinterpret_cast<const V*>(Lk + (int64_t)(r0 + u) * lds_ + out[u]);
        }
      };
      auto fma8 = [&](const V (&lv)[8], const int (&out)[8], int r0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const T xv = out[u] > 0 ? T(0) : xb[r0 + u];
          // (explicit fused multiply-adds: -ffp-contract leaves the choice to the vectoriser, which mixes packed multiplies +
          //  adds into the chain -- the block-row kernel below must reproduce this sum bit for bit)
          if constexpr (sizeof(T) == 4) {
            s[0] = fma_t(lv[u].x, xv, s[0]); s[1] = fma_t(lv[u].y, xv, s[1]); s[2] = fma_t(lv[u].z, xv, s[2]); s[3] = fma_t(lv[u].w, xv, s[3]);
          } else {
            s[0] = fma_t(lv[u].x, xv, s[0]); s[1] = fma_t(lv[u].y, xv, s[1]);
          }
        }
      };
      int rr = 0;
      V la[8];
      int oa[8];
      if constexpr (ENV) {
        // Two groups of eight rows in flight: the lanes left of a row's envelope hold a load slot without bringing new bytes, so
        // with one group in flight the kernel fell from the memory bound to the latency bound (15.05 GB in 3.16 ms = 4.8 TB/s
        // where the plain kernel streams 6.2).  The next group's loads are issued before the current group's multiply-adds.
        const int ng = valid / 8;
        if (ng > 0) {
          V lb[8];
          int ob[8];
          load8(la, oa, 0);
          int g = 0;
          for (; g + 2 < ng; g += 2) {
            load8(lb, ob, 8 * (g + 1));
            fma8(la, oa, 8 * g);
            load8(la, oa, 8 * (g + 2));
            fma8(lb, ob, 8 * (g + 1));
          }
          if (g + 1 < ng) {   // two groups left (la holds the first), or one
            load8(lb, ob, 8 * (g + 1));
            fma8(la, oa, 8 * g);
            fma8(lb, ob, 8 * (g + 1));
          } else {
            fma8(la, oa, 8 * g);
          }
          rr = 8 * ng;
        }
      } else {
        for (; rr + 8 <= valid; rr += 8) {
          load8(la, oa, rr);
          fma8(la, oa, rr);
        }
      }
      for (; rr < valid; ++rr) {
        const int out = ENV ? max(fb[rr] - k, 0) : 0;
        const V lv = *reinterpret_cast<const V*>(Lk + (int64_t)rr * lds_ + out);
        const T xv = out > 0 ? T(0) : xb[rr];
        if constexpr (sizeof(T) == 4) {
          s[0] = fma_t(lv.x, xv, s[0]); s[1] = fma_t(lv.y, xv, s[1]); s[2] = fma_t(lv.z, xv, s[2]); s[3] = fma_t(lv.w, xv, s[3]);
        } else {
          s[0] = fma_t(lv.x, xv, s[0]); s[1] = fma_t(lv.y, xv, s[1]);
        }
      }
      if constexpr (LIST) {   // (scalar accesses: a row of the vector need not be 16-byte aligned, ldv = n = 6 P)
#pragma unroll
        for (int u = 0; u < C::VEC; ++u) zg[k + u] -= s[u];
      } else {
#pragma unroll
        for (int u = 0; u < C::VEC; ++u) z[k + u] -= s[u];
      }
    }
    __syncthreads();
  }
  if constexpr (!LIST)
    for (int k = tid; k < n; k += 256) x[(int64_t)b * ldv + k] = z[k];
}

// L^T x = y for SMALL batches on dense frames, one launch per block row instead of one workgroup per problem (round 6):
// chol_bwd_kernel streams a problem's whole lower triangle through ONE workgroup.  Here block row jb is its own launch, x is the
// working vector (z) in place:
//   workgroup (k, b), k < jb:  z_k -= L_jb,k^T x_jb   (x_jb is final: the previous launch finished it) -- and the workgroup of
//   k = jb - 1 then holds the finished z_jb-1 (rows above jb pushed into it in earlier launches: stream order) and turns it into
//   x_jb-1 = L_jj^-T z_jb-1 through the panel, in place: the only writer of that block in this launch.
// The first launch (jb = ntiles) only finishes the last block.  Per column the same sums in the same order as chol_bwd_kernel
// (rows ascending, fused multiply-adds; the same panel substitution): the solution is bit-identical.
template <typename T>
__global__ void __launch_bounds__(256)
chol_bwd_rows_kernel(const T* __restrict__ L, const T* __restrict__ panel, T* __restrict__ x, int n, int64_t ld, int64_t ldv,
                     int ntiles, int jb) {
  using C = CT<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tile = reinterpret_cast<T*>(smem_raw);
  T* xb = tile + 128 * C::LDM;   // [128]
  T* ubuf = xb + 128;            // [32]
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  T* xg = x + (int64_t)b * ldv;
  if (jb < ntiles) {   // push of block row jb into column block k
    const int row0 = jb * TILE, valid = min(TILE, n - row0);
    if (tid < TILE) xb[tid] = tid < valid ? xg[row0 + tid] : T(0);
    __syncthreads();
    if (tid < TILE) {
      const T* Lk = L + (int64_t)b * ld * ld + (int64_t)row0 * ld + k * TILE + tid;
      T s = T(0);
      int rr = 0;
      for (; rr + 16 <= valid; rr += 16) {
        T lv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) lv[u] = Lk[(int64_t)(rr + u) * ld];
        // (explicit fused multiply-adds: left to -ffp-contract the vectoriser emits packed multiplies + separate adds for half of
        //  the chain -- other roundings than chol_bwd_kernel's v_fmac chain)
#pragma unroll
        for (int u = 0; u < 16; ++u) s = fma_t(lv[u], xb[rr + u], s);
      }
      for (; rr < valid; ++rr) s = fma_t(Lk[(int64_t)rr * ld], xb[rr], s);
      xg[k * TILE + tid] -= s;
    }
    if (k != jb - 1) return;   // (workgroup uniform)
    __syncthreads();           // block jb - 1 of x is finished and visible to this workgroup (its own writes)
  } else if (k != 0) {
    return;
  }
  // finish block jf = jb - 1: x_jf = L_jf,jf^-T z_jf through the panel
  const int jf = jb - 1, row0 = jf * TILE, valid = min(TILE, n - row0);
  panel_g2l<T>(panel + ((int64_t)b * ntiles + jf) * TILE * TILE, tile, tid);
  if (tid < TILE) xb[tid] = tid < valid ? xg[row0 + tid] : T(0);
  __syncthreads();
  if (wave == 0) panel_backward<T>(tile, xb, ubuf, lane);
  __syncthreads();
  if (tid < valid) xg[row0 + tid] = xb[tid];
}

}  // namespace thx
