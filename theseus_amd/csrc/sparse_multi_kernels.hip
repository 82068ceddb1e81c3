// Triangular solves with a BLOCK of right-hand sides against a TILE-SPARSE Cholesky factor, for gfx950:
//   X = (L L^T)^-1 R,  X = L^-T R  or  X = L^-1 R   for R = (B, nrhs, n), one vector per row,
// with L as thx_chol_factor_sparse / thx_chol_factor_hblocks (with a pattern) / thx_chol_factor_levels leave it: the tile pattern on
// a dense frame (ld > 0), the tile-packed factor (ld = 0) or the padded, level-ordered tile-packed factor (ld = 0 and tile_row0).
// What HipSparseCholeskySolver needs for posterior samples and marginal covariances of the graphs whose dense frame cannot exist;
// the single-vector thx_chol_solve_sparse streams every non-zero tile once per vector with scalar dot products.
//
// One 256-thread workgroup per (problem, group of 32 right-hand sides), as in multi_solve_kernels.hip; the block of vectors stays
// in x (global memory / L2).  On chip: the accumulator of the current 128 x 32 block (a 32 x 32 fragment per wave), one 128 x 32
// chunk of L in LDS (sA) and the X operand in LDS (sX: 32 rows of it forward, the whole finished block row backward).
//   forward, block row i ascending -- PULL along the row list of i:
//     T = R_i - sum_k L_ik X_k over the listed tiles (i, k), k ascending: 32-column chunks of L_ik (A) x 32 rows of X_k (B);
//     then through the Winv panel of tile i, 32 rows at a time:  x_s = W_ss t_s ;  t_u += (-L_us) x_s, u > s.
//   backward, block row i descending -- PUSH along the same row list:
//     T = X_i as the pushes of the rows below left it;  x_s = W_ss^T t_s ;  t_u += (-L_su)^T x_s, u < s, s = 3..0;  X_i stays in sX;
//     for every listed tile (i, k):  X_k -= L_ik^T X_i -- the accumulator starts from X_k in global memory, 32-ROW chunks of the
//     tile are read as they lie and used transposed, X_k goes back.  No column lists: one kernel serves TilePattern and LevelPattern.
// Ascending / descending block rows are a valid elimination order for every pattern (the row list of i names tiles k < i only).
// Tile j holds the matrix rows row0(j) .. row0(j) + valid(j) in its first rows: tile_row0[j] .. tile_row0[j + 1], or, without
// the table, 128 j .. min(128 j + 128, n).  Rows and columns of a tile or panel beyond valid are masked as they are loaded; tiles
// the lists do not name are never read.  The next chunk is in flight in registers while the matrix cores work on the current one.
// The workgroup re-reads blocks of x it wrote itself: a barrier stands in front of every such read, and x is not __restrict__.
#include <cstdint>

#include "common.cuh"
#include "multi_solve_mma.cuh"

namespace thx {

template <typename T>
struct SmsFactor {
  const T* L;              // this problem's frame / slots
  const T* P;              // this problem's Winv panels
  int64_t ld;              // 0: tile-packed
  int n, nt;
  const int32_t *row_ptr, *row_tile, *row_slot, *tile_row0;
  __device__ __forceinline__ int row0(int j) const { return tile_row0 ? min(max(tile_row0[j], 0), n) : MS_TILE * j; }
  __device__ __forceinline__ int valid(int j) const {
    const int r0 = row0(j);
    return tile_row0 ? min(max(tile_row0[j + 1] - r0, 0), min(MS_TILE, n - r0)) : min(MS_TILE, n - r0);
  }
  // listed tile e of block row i (block column k): its first element and its row stride
  __device__ __forceinline__ const T* tile(int e, int i, int k) const {
    return ld ? L + (int64_t)MS_TILE * i * ld + MS_TILE * k : L + (int64_t)row_slot[e] * MS_TILE * MS_TILE;
  }
  __device__ __forceinline__ int64_t stride() const { return ld ? ld : MS_TILE; }
};

// Chunk c of a 128 x 128 tile (row stride ls) -> registers.  TR = false: its columns 32 c .. 32 c + 31, all rows; TR = true: its rows
// 32 c .. 32 c + 31, all columns.  Rows >= vr are not read, columns >= vc are dropped: both come out as zeros.
template <typename T, bool TR>
__device__ __forceinline__ void sms_load(typename MsVec<T>::V (&ra)[MS_TILE * MS_KC / MsVec<T>::NV / 256], const T* tile, int64_t ls,
                                         int c, int vr, int vc, int tid) {
  using VT = MsVec<T>;
  using V = typename VT::V;
  constexpr int NV = VT::NV, NL = MS_TILE * MS_KC / NV / 256, VPR = (TR ? MS_TILE : MS_KC) / NV;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int v = tid + 256 * u, a = v / VPR, bq = (v % VPR) * NV;   // element (a, bq..) of the chunk as it lies in memory
    const int r = TR ? MS_KC * c + a : a, q = TR ? bq : MS_KC * c + bq;
    V val = VT::zero();
    if (r < vr) {
      const V pv = *reinterpret_cast<const V*>(tile + (int64_t)r * ls + q);
      T e[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) e[i] = (q + i < vc) ? VT::at(pv, i) : T(0);
      if constexpr (NV == 4) val = V{e[0], e[1], e[2], e[3]};
      else val = V{e[0], e[1]};
    }
    ra[u] = val;
  }
}

template <typename T, bool TR>
__device__ __forceinline__ void sms_store(T* sA, const typename MsVec<T>::V (&ra)[MS_TILE * MS_KC / MsVec<T>::NV / 256], int tid) {
  using VT = MsVec<T>;
  constexpr int NV = VT::NV, NL = MS_TILE * MS_KC / NV / 256, VPR = (TR ? MS_TILE : MS_KC) / NV;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int v = tid + 256 * u, a = v / VPR, bq = (v % VPR) * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) sA[a * (TR ? MS_LST : MS_LSA) + bq + i] = VT::at(ra[u], i);
  }
}

__device__ __forceinline__ int sms_chunks(int valid) { return max((valid + MS_KC - 1) / MS_KC, 1); }

// out = L^-1 in.  `in` is read one block row at a time, just before that block row of `out` is written: out may be in.
template <typename T>
__device__ __forceinline__ void sms_forward(const SmsFactor<T>& F, const T* in, T* out, int nc, int64_t ldv, T* sA, T* sX, int tid) {
  using M = MsMma<T>;
  using V = typename MsVec<T>::V;
  constexpr int NL = MS_TILE * MS_KC / MsVec<T>::NV / 256;
  const int wave = tid >> 6, lane = tid & 63;
  const int bs = tid >> 3, bk = (tid & 7) * 4;         // this thread's vector and first row of a chunk of X
  const int64_t ls = F.stride();

  for (int ib = 0; ib < F.nt; ++ib) {
    const int row0 = F.row0(ib), valid = F.valid(ib);
    const int e0 = F.row_ptr[ib], e1 = F.row_ptr[ib + 1];
    int nch = 0;                                       // chunks of the listed tiles; then the four of the panel
    for (int e = e0; e < e1; ++e) nch += sms_chunks(F.valid(F.row_tile[e]));
    const T* Pn = F.P + (int64_t)ib * MS_TILE * MS_TILE;
    V ra[NL];
    T rb[4];
    // the load side's place in the list: tile le, its chunk lc
    int le = e0, lc = 0, lvk = 0, lxk = 0;
    const T* lt = nullptr;
    auto open = [&]() __attribute__((always_inline)) {
      if (le < e1) {
        const int k = F.row_tile[le];
        lt = F.tile(le, ib, k);
        lvk = F.valid(k);
        lxk = F.row0(k);
      }
    };
    open();
    auto load = [&](int c) __attribute__((always_inline)) {
      if (c >= nch) {
        sms_load<T, false>(ra, Pn, MS_TILE, c - nch, valid, valid, tid);
        return;
      }
      sms_load<T, false>(ra, lt, ls, lc, valid, lvk, tid);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = MS_KC * lc + bk + i;
        rb[i] = (bs < nc && k < lvk) ? out[(int64_t)bs * ldv + lxk + k] : T(0);
      }
      if (++lc == sms_chunks(lvk)) {
        ++le;
        lc = 0;
        open();
      }
    };

    typename M::Frag acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) M::set(acc, e, T(0));
    load(0);
    for (int c = 0; c < nch + 4; ++c) {
      __syncthreads();   // the previous chunk has been consumed; block rows of `out` written so far are visible to the workgroup
      const bool diag = c >= nch;
      const int s = c - nch;
      if (c == nch) {    // T = in_i - (product accumulated from zero)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = MS_KC * wave + M::row(e, lane), j = M::col(e, lane);
          const T v = (r < valid && j < nc) ? in[(int64_t)j * ldv + row0 + r] : T(0);
          M::set(acc, e, v - M::get(acc, e));
        }
      }
      sms_store<T, false>(sA, ra, tid);
      if (!diag) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sX[(bk + i) * MS_LSB + bs] = rb[i];
      } else if (wave == s) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sX[M::row(e, lane) * MS_LSB + M::col(e, lane)] = M::get(acc, e);
      }
      __syncthreads();
      if (c + 1 < nch + 4) load(c + 1);
      const T* sAw = sA + MS_KC * wave * MS_LSA;   // this wave's 32 rows of the block row
      if (!diag) {
        M::template mac<MS_LSA, 1>(acc, sAw, sX, lane);
      } else {
        // x_s = W_ss t_s by wave s, then t_u += (-L_us) x_s by the waves still open
        if (wave == s) {
          typename M::Frag xs;
#pragma unroll
          for (int e = 0; e < 16; ++e) M::set(xs, e, T(0));
          M::template mac<MS_LSA, 1>(xs, sAw, sX, lane);
          acc = xs;
        }
        __syncthreads();   // t_s has been read by all lanes of wave s
        if (wave == s) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = M::row(e, lane), j = M::col(e, lane), r = MS_KC * s + rl;
            const T v = M::get(acc, e);
            sX[rl * MS_LSB + j] = v;
            if (r < valid && j < nc) out[(int64_t)j * ldv + row0 + r] = v;
          }
        }
        __syncthreads();
        if (wave > s) M::template mac<MS_LSA, 1>(acc, sAw, sX, lane);
      }
    }
  }
}

// x = L^-T x, in place: block row i is finished through its panel once the rows below have pushed their products into it.
template <typename T>
__device__ __forceinline__ void sms_backward(const SmsFactor<T>& F, T* x, int nc, int64_t ldv, T* sA, T* sX, int tid) {
  using M = MsMma<T>;
  using V = typename MsVec<T>::V;
  constexpr int NL = MS_TILE * MS_KC / MsVec<T>::NV / 256;
  const int wave = tid >> 6, lane = tid & 63;
  const int64_t ls = F.stride();

  for (int ib = F.nt - 1; ib >= 0; --ib) {
    const int row0 = F.row0(ib), valid = F.valid(ib);
    const int e0 = F.row_ptr[ib], e1 = F.row_ptr[ib + 1];
    const int npc = sms_chunks(valid);                 // 32-row chunks of a listed tile
    const int total = 4 + (e1 - e0) * npc;             // the four of the panel, then the listed tiles
    const T* Pn = F.P + (int64_t)ib * MS_TILE * MS_TILE;
    V ra[NL];
    auto load = [&](int c) __attribute__((always_inline)) {
      if (c < 4) {
        sms_load<T, true>(ra, Pn, MS_TILE, 3 - c, valid, valid, tid);
        return;
      }
      const int e = e0 + (c - 4) / npc, k = F.row_tile[e];
      sms_load<T, true>(ra, F.tile(e, ib, k), ls, (c - 4) % npc, valid, F.valid(k), tid);
    };

    typename M::Frag acc;
    int xk0 = 0, vk = 0;                               // the block row of x that the current tile's product goes to
    load(0);
    for (int c = 0; c < total; ++c) {
      __syncthreads();   // the previous chunk has been consumed; what the workgroup stored into x is visible to it
      const bool diag = c < 4;
      const int s = 3 - c, pc = diag ? 0 : (c - 4) % npc;
      if (c == 0) {      // T = X_i
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = MS_KC * wave + M::row(e, lane), j = M::col(e, lane);
          M::set(acc, e, (r < valid && j < nc) ? x[(int64_t)j * ldv + row0 + r] : T(0));
        }
      }
      sms_store<T, true>(sA, ra, tid);
      if (diag && wave == s) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sX[(MS_KC * s + M::row(e, lane)) * MS_LSB + M::col(e, lane)] = M::get(acc, e);
      }
      if (!diag && pc == 0) {   // -X_k: the product is added to it and the sum negated on its way back
        const int k = F.row_tile[e0 + (c - 4) / npc];
        xk0 = F.row0(k);
        vk = F.valid(k);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = MS_KC * wave + M::row(e, lane), j = M::col(e, lane);
          M::set(acc, e, (r < vk && j < nc) ? -x[(int64_t)j * ldv + xk0 + r] : T(0));
        }
      }
      __syncthreads();
      if (c + 1 < total) load(c + 1);
      const T* sAw = sA + MS_KC * wave;            // this wave's 32 columns of the chunk = its 32 rows of the product
      if (!diag) {
        M::template mac<1, MS_LST>(acc, sAw, sX + MS_KC * pc * MS_LSB, lane);
        if (pc == npc - 1) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int r = MS_KC * wave + M::row(e, lane), j = M::col(e, lane);
            if (r < vk && j < nc) x[(int64_t)j * ldv + xk0 + r] = -M::get(acc, e);
          }
        }
      } else {
        // x_s = W_ss^T t_s by wave s, then t_u += (-L_su)^T x_s by the waves still open
        T* sXs = sX + MS_KC * s * MS_LSB;
        if (wave == s) {
          typename M::Frag xs;
#pragma unroll
          for (int e = 0; e < 16; ++e) M::set(xs, e, T(0));
          M::template mac<1, MS_LST>(xs, sAw, sXs, lane);
          acc = xs;
        }
        __syncthreads();   // t_s has been read by all lanes of wave s
        if (wave == s) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = M::row(e, lane), j = M::col(e, lane), r = MS_KC * s + rl;
            const T v = M::get(acc, e);
            sXs[rl * MS_LSB + j] = v;
            if (r < valid && j < nc) x[(int64_t)j * ldv + row0 + r] = v;
          }
        }
        __syncthreads();
        if (wave < s) M::template mac<1, MS_LST>(acc, sAw, sXs, lane);
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
chol_solve_multi_sparse_kernel(const T* __restrict__ L, int64_t ld, int64_t lstride, int n, int nt, const T* __restrict__ Winv,
                               const T* rhs, T* x, int nrhs, int64_t ldv, int64_t bstride, int ngroups, int fwd, int bwd,
                               const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ row_tile,
                               const int32_t* __restrict__ row_slot, const int32_t* __restrict__ tile_row0) {
  __shared__ __attribute__((aligned(16))) T sA[MS_SA];
  __shared__ T sX[MS_TILE * MS_LSB];
  const int b = blockIdx.x / ngroups, g = blockIdx.x % ngroups, tid = threadIdx.x;
  const int nc = min(MS_G, nrhs - MS_G * g);
  const SmsFactor<T> F{L + (int64_t)b * lstride, Winv + (int64_t)b * nt * MS_TILE * MS_TILE, ld, n, nt,
                       row_ptr, row_tile, row_slot, tile_row0};
  const T* in = rhs + (int64_t)b * bstride + (int64_t)MS_G * g * ldv;
  T* out = x + (int64_t)b * bstride + (int64_t)MS_G * g * ldv;
  if (fwd) {
    sms_forward<T>(F, in, out, nc, ldv, sA, sX, tid);
  } else if (in != out) {   // the backward pass works in place
    for (int j = 0; j < nc; ++j)
      for (int r = tid; r < n; r += 256) out[(int64_t)j * ldv + r] = in[(int64_t)j * ldv + r];
  }
  if (bwd) sms_backward<T>(F, out, nc, ldv, sA, sX, tid);
}

template <typename T>
static int solve_multi_sparse_impl(const void* L, int64_t ld, int n, int B, const void* Winv, const void* rhs, void* x, int nrhs,
                                   int64_t ldv, int64_t bstride, int which, const thx_tile_pattern* tp, const int32_t* tile_row0,
                                   hipStream_t st) {
  const int ngroups = (int)(((int64_t)nrhs + MS_G - 1) / MS_G);
  const int64_t lstride = ld ? ld * ld : (int64_t)tp->nslots * MS_TILE * MS_TILE;
  chol_solve_multi_sparse_kernel<T><<<dim3((unsigned)(B * ngroups)), dim3(256), 0, st>>>(
      static_cast<const T*>(L), ld, lstride, n, tp->ntiles, static_cast<const T*>(Winv), static_cast<const T*>(rhs), static_cast<T*>(x),
      nrhs, ldv, bstride, ngroups, which != 1, which != 2, tp->row_ptr, tp->row_tile, ld ? nullptr : tp->row_slot, tile_row0);
  return check_launch("thx_chol_solve_multi_sparse");
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_chol_solve_multi_sparse(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x, int32_t nrhs,
                                int64_t ldv, int64_t bstride, int which, const thx_tile_pattern* pattern, const int32_t* tile_row0,
                                int dtype, void* stream) {
  const char* who = "thx_chol_solve_multi_sparse";
  if (!L || !Winv || !rhs || !x || !pattern) return fail(who, ": null pointer");
  if (n <= 0 || B <= 0) return fail(who, ": need n>0, B>0");
  if (ld != 0 && (ld < n || (ld % 32) != 0)) return fail(who, ": ld = 0 (tile-packed factor) or a dense frame, ld>=n, ld%32==0");
  if (!pattern->row_ptr || !pattern->row_tile || (ld == 0 && !pattern->row_slot)) return fail(who, ": incomplete tile pattern");
  if (ld == 0 && pattern->nslots < pattern->ntiles) return fail(who, ": a tile-packed factor (ld = 0) needs nslots >= ntiles");
  if (tile_row0 && ld != 0) return fail(who, ": tile_row0 (padded tiles) goes with the tile-packed factor, ld = 0");
  if (tile_row0 ? (pattern->ntiles < 1 || (int64_t)pattern->ntiles * MS_TILE < n) : pattern->ntiles != (n + MS_TILE - 1) / MS_TILE)
    return fail(who, ": the pattern is not this matrix's");
  if (nrhs < 1) return fail(who, ": nrhs < 1");
  if (ldv < n) return fail(who, ": ldv < n");
  if (bstride / nrhs < ldv) return fail(who, ": bstride < nrhs * ldv");   // (no product: nrhs * ldv may not fit)
  if (which < 0 || which > 2) return fail(who, ": which = 0 (both), 1 (backward only), 2 (forward only)");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if ((reinterpret_cast<uintptr_t>(L) | reinterpret_cast<uintptr_t>(Winv)) % 16) return fail(who, ": L and Winv must be 16-byte aligned");
  if ((int64_t)B * (((int64_t)nrhs + MS_G - 1) / MS_G) > 0x7fffffffLL) return fail(who, ": B * ceil(nrhs / 32) exceeds the grid limit");
  THX_DISPATCH(dtype,
               return solve_multi_sparse_impl<float>(L, ld, n, B, Winv, rhs, x, nrhs, ldv, bstride, which, pattern, tile_row0,
                                                     as_stream(stream)),
               return solve_multi_sparse_impl<double>(L, ld, n, B, Winv, rhs, x, nrhs, ldv, bstride, which, pattern, tile_row0,
                                                      as_stream(stream)));
  return 0;
}

}  // extern "C"
