#pragma once
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_engine.cuh"
#include "chol_potrf.cuh"

namespace thx {

// device view of thx_tile_pattern (include/theseus_hip.h): which 128x128 tiles of L are structurally non-zero
struct TilePat {
  const int32_t* col_ptr;    // (ntiles + 1) entries of block column j: [col_ptr[j], col_ptr[j + 1])
  const int32_t* col_row;    // row tile of every entry (ascending within a column)
  const int32_t* tile_kptr;  // (entries + 1) K-list of entry e ...
  const int32_t* tile_k;     // ... block columns k < j in which L_ik and L_jk are both non-zero
  const int32_t* diag_kptr;  // (ntiles + 1) K-list of diagonal tile j ...
  const int32_t* diag_k;     // ... block columns k < j with L_jk non-zero
  // TILE-PACKED factor (nslots > 0): L is (B, nslots, TILE, TILE) -- only the tiles of the pattern exist: slot j = diagonal tile
  // j, slot ntiles + e = off-diagonal entry e -- and every K-list element carries the slots of its two operand tiles
  const int32_t* tile_sa;    // (per tile_k element) slot of L_jk
  const int32_t* tile_sb;    //                      slot of L_ik
  const int32_t* diag_s;     // (per diag_k element) slot of L_jk
  int32_t nslots;            // 0: L is the dense (B, ld, ld) frame
  int32_t lpt;               // chol_offdiag's block -> (problem, entry) map: 1 = the ENTRY is the slow index (longest K-lists first)
  // LEVEL schedule (thx_chol_factor_levels): one launch covers every block column of an elimination-tree level
  const int32_t* ent_col;    // (entries) block column of entry e -- the launch's entries then are [i_first, i_first + nrow_tiles)
  const int32_t* tile_valid; // (ntiles) rows / columns of tile j inside the matrix, the rest is identity padding (per-tile padding:
                             // no variable straddles a tile boundary); nullptr: min(TILE, n - j * TILE)
  // RIGHT-LOOKING schedule of small dense batches (factor_impl: "rl"): 0 = the left-looking kernels as they are; 1 = no K-loop
  // (the tile read from the H argument already carries every earlier column's update: chol_diag = the tile factorisation alone,
  // chol_offdiag = the substitution alone); 2 + jc = chol_offdiag as the TRAILING UPDATE of block column jc: workgroup slot t ->
  // tile (i, k), jc < k <= i, receives  A_ik - L_i,jc L_k,jc^T  (no substitution), written to the L frame
  int32_t rl;
  // right-looking schedule with a right-hand side: the vector being forward-substituted, (B, rl_ldv) -- g on entry; chol_diag
  // turns block j into y_j in place, every substitution tile (i, j) then takes  L_ij y_j  off block i (chol_offdiag, rl == 1)
  void* rl_y;
  int64_t rl_ldv;
  // right-looking schedule, two launches per block column (rl == 1): the tile takes the PREVIOUS block column's update itself -- a
  // K-loop over the one tile of column j - 1, the left-looking kernels' own path -- instead of finding it applied: chol_diag(j)
  // and the substitution tiles (i, j) of chol_offdiag
  int32_t rl_la;
  // ... and ONE chol_offdiag launch per block column (rl == 1, rl_la == 1, rl_nsub > 0): slots [0, rl_nsub) = the substitution
  // tiles (i, jarg), each taking column jarg - 1's update of itself first (a K-loop over the one tile of that column); the other
  // slots = column jarg - 1's trailing update of the tiles (i, k), jarg < k <= i -- which nobody needs before column jarg + 1
  int32_t rl_nsub;
};

// rows (= columns) of diagonal tile j that belong to the matrix
__device__ __forceinline__ int tile_rows(const TilePat& pat, int n, int j) {
  return pat.tile_valid ? pat.tile_valid[j] : min(TILE, n - j * TILE);
}

// where a kernel finds / puts the tiles of L: the dense frame (row stride ld) or the tile-packed buffer (row stride TILE)
struct LFrame {
  int64_t pstride;   // elements per problem
  int64_t ld;        // row stride of a tile
  bool packed;
  __device__ __forceinline__ int64_t tile(int ti, int tj, int slot) const {   // element offset of tile (ti, tj) inside a problem
    return packed ? (int64_t)slot * TILE * TILE : (int64_t)ti * TILE * ld + (int64_t)tj * TILE;
  }
};
__device__ __forceinline__ LFrame lframe(const TilePat& pat, int64_t ld) {
  const bool packed = pat.nslots > 0;
  return LFrame{packed ? (int64_t)pat.nslots * TILE * TILE : ld * ld, packed ? (int64_t)TILE : ld, packed};
}

// Fused forward substitution through a finished panel column (sub-block column sb of the diagonal tile), on blocks in the
// register layout of Engine::Blk:  y_s = W_ss u_s ;  u_u += (-L_us) y_s  for the sub-blocks below.  ONE implementation for both
// schedules of the diagonal phase (chol_diag_kernel loads the blocks from its LDS tile, chol_potrf_kernel has them in
// registers): the same sums in the same order, so y -- and with it every LM trajectory -- does not depend on which schedule a
// batch size selects (tests/test_gpu_full_size.py: any slice of a batch solved alone is bit-identical).
template <typename T>
__device__ __forceinline__ void fwd_diag_block(const typename Engine<T>::Blk& W, T* vvec, int sb, int lane) {
  using E = Engine<T>;
  T y[E::NR];
  E::blk_rowdot(W, vvec + 32 * sb, lane, y);
  wave_lds_fence();   // every lane has read u_s
  if (E::row_owner(lane)) {
#pragma unroll
    for (int i = 0; i < E::NR; ++i) vvec[32 * sb + E::blk_row(lane, i)] = y[i];
  }
  wave_lds_fence();
}
template <typename T>
__device__ __forceinline__ void fwd_below_block(const typename Engine<T>::Blk& X, T* vvec, int sb, int u, int lane) {
  using E = Engine<T>;
  T part[E::NR];
  E::blk_rowdot(X, vvec + 32 * sb, lane, part);
  if (E::row_owner(lane)) {
#pragma unroll
    for (int i = 0; i < E::NR; ++i) vvec[32 * u + E::blk_row(lane, i)] += part[i];
  }
}

// device view of a block-compact Hessian (include/theseus_hip.h: thx_hblock_layout + the value buffer); blocks == nullptr:
// H is the dense frame
struct HBlk {
  const void* blocks;
  int64_t bstride;
  int bd;
  const int32_t* tile_ptr;
  const int32_t* piece_blk;
  const int32_t* piece_rc;
  const int32_t* diag_blk;   // (nvars) block id of variable v's diagonal block (the right-looking schedule's damping pass; may be null)
  int max_tile_pieces;       // thx_hblock_layout.max_tile_pieces (host side: picks the off-diagonal kernels' HB mode); 0: unknown
  // thx_hblock_layout.l_mask: (ntiles, 4 * ntiles) 4-bit masks of the structurally non-zero 32-row sub-blocks of tile t at 32-column
  // chunk c -- set by factor_impl only for the fp32 column-by-column dense-frame schedule (FactorPlan.zskip), nullptr otherwise
  const int32_t* l_mask;
  // thx_hblock_layout.rg_*: the row groups of the fp32 column pairs (chol_offdiag2_f32_kernel<HB, true>) -- set by factor_impl only
  // with FactorPlan.regroup, nullptr otherwise
  const int32_t* rg_rows;
  const int32_t* rg_k0;
  const int32_t* rg_tile_ptr;
  const int32_t* rg_piece_blk;
  const int32_t* rg_piece_rc;
  const int32_t* rg_group_ptr_host;   // (HOST table: run_left_looking sizes the launches by it; no kernel reads it)
  int rg_max_tile_pieces;
  // thx_hblock_layout.rg_zf: per (group, wave) the first non-zero chunk of the wave's 32 rows -- set by factor_impl only with
  // FactorPlan.zsolve, nullptr otherwise (pair_groups0 puts pair 0's table here)
  const int32_t* rg_zf;
  // thx_hblock_layout.rg0_*: pair 0's groups (HOST side only: pair_groups0 moves them into the rg_ fields of its launch)
  const int32_t* rg0_rows;
  const int32_t* rg0_zf;
  const int32_t* rg0_tile_ptr;
  const int32_t* rg0_piece_blk;
  const int32_t* rg0_piece_rc;
  int rg0_ngroups;
  int rg0_max_tile_pieces;
  // thx_hblock_layout.sc_*: the sorted columns of the fp32 column pairs (chol_offdiag2_f32_kernel<HB, true, true>, the only kernel
  // that reads them) -- set by factor_impl only with FactorPlan.sortcols, nullptr otherwise; pair_groups points sc_perm / sc_mask
  // at the tables of the launch's OWN pair
  const int32_t* sc_perm;        // (256) sorted slot -> column of the pair, 0 .. 255
  const int32_t* sc_mask;        // (4 ntiles) per k-chunk the 8-bit mask of the active sorted blocks
  const int32_t* sc_pair_host;   // (HOST table, npairs: the pair has tables; no kernel reads it)
  // thx_hblock_layout.tr_*: the sorted rows of the diagonal tiles (chol_syrk_kernel<float, true, true>, the only kernel that reads
  // them) -- set by factor_impl only with FactorPlan.sortrows, nullptr otherwise
  const int32_t* tr_perm16;      // (ntiles, 128) staged slot -> row of tile j, 0 .. 127
  const int32_t* tr_mask16;      // (ntiles, 4 ntiles) per k-chunk the 8-bit mask of the active staged block rows of 16
  const int32_t* tr_tile_host;   // (HOST table, ntiles: the tile has tables; no kernel reads it)
  // thx_hblock_layout.th_*: the sorted columns of the head tiles (j + 1, j) (chol_offdiag_f32_kernel<HB, true>, the only kernel that
  // reads them) -- set by factor_impl only with FactorPlan.sorthead, nullptr otherwise
  const int32_t* th_perm32;      // (ntiles, 128) sorted slot -> row of tile j, 0 .. 127
  const int32_t* th_mask32;      // (ntiles, 4 ntiles) per k-chunk the 4-bit mask of the active sorted blocks of 32
  const int32_t* th_k0h;         // (ntiles) first k-chunk of the head tile's K-loop
  const int32_t* th_tile_host;   // (HOST table, ntiles: tile j's head tile has tables; no kernel reads it)
};

// The pieces of lower tile (ti, tj) of problem b -- f(r, c, value), (r, c) relative to the tile origin and inside the tile; the
// blocks of a tile are one contiguous run of the list (straddlers from the neighbours aside): coalesced reads -- fetched EARLY:
// the first NPRE x 256 elements of the tile go global -> registers in the kernel's prologue (two
// dependent loads each -- table, then value: ~2 us if left to the epilogue, measured as +1.3 ms per factorisation), the K-loop
// hides them; ``foreach`` then replays them from registers (and walks whatever is beyond NPRE x 256 from memory).
template <typename T, int NPRE, int NT = 256>   // (NT: threads of the workgroup)
struct HBPre {
  static constexpr int CAP = NT * NPRE;   // elements the registers hold
  T v[NPRE];
  int rc[NPRE];   // (r << 8) | c inside the tile, -1: nothing
  int p0, cnt;
  int wmeta;      // lane l of every wave: piece_rc of the tile's piece l (hb_scatter: readlane)
  // the tile's elements, in list order, -> LDS (element idx of the tile's run at list[idx]; the caller publishes them with a barrier)
  __device__ __forceinline__ void to_list(T* list, int tid) const {
#pragma unroll
    for (int k = 0; k < NPRE; ++k)
      if (tid + NT * k < cnt) list[tid + NT * k] = v[k];   // (k < NPRE: what the registers hold)
  }
  // BRANCH-FREE (round 5): the loads of all NPRE elements are independent of each other -- with an ``if (idx < cnt)`` around each
  // element hipcc emitted  table load, s_waitcnt vmcnt(0), table load, s_waitcnt vmcnt(0), value load  once per element, i.e.
  // 2 NPRE exposed round trips at the head of every workgroup (6 per off-diagonal tile, 14 per SYRK workgroup).  Now: both tables
  // of all elements in one batch, one wait, all values in one batch whose wait is the first use (after the K-loop).  A lane
  // without an element reads element 0 of the tile's first piece and discards it.
  // (Round 6 measured the chain in TWO PHASES -- tile_ptr -> piece_rc / piece_blk at the kernel's very top, the values behind the
  //  first k-chunk's loads: no gain in fp64, 0.4 of 43.5 ms SLOWER in fp32, profiles/r6/ab_.  load() keeps both in one place; the
  //  split stays as two functions.)
  int tw[NPRE], tblk[NPRE];   // (live between the phases only)
  __device__ __forceinline__ void load_tables(const HBlk& hb, int ti, int tj, int tid) {
    const int bd = hb.bd, bb = bd * bd, t = ti * (ti + 1) / 2 + tj;
    p0 = hb.tile_ptr[t];
    cnt = (hb.tile_ptr[t + 1] - p0) * bb;
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      rc[k] = -1;
      v[k] = T(0);
      tw[k] = tblk[k] = 0;
    }
    wmeta = 0;
    if (cnt <= 0) return;   // (workgroup uniform; p0 may be the END of the piece list)
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int idx = tid + NT * k;
      const int pc = p0 + (idx < cnt ? idx : 0) / bb;
      tw[k] = hb.piece_rc[pc];
      tblk[k] = hb.piece_blk[pc];
    }
    wmeta = hb.piece_rc[p0 + min(tid & 63, cnt / bb - 1)];
  }
  // BRANCH-FREE (round 5): the loads of all NPRE elements are independent of each other -- all values in one batch whose wait is
  // the first use (after the K-loop).  A lane without an element reads element 0 of the tile's first piece and discards it.
  __device__ __forceinline__ void load_values(const HBlk& hb, int b, int tid) {
    if (cnt <= 0) return;
    const T* base = static_cast<const T*>(hb.blocks) + (int64_t)b * hb.bstride;
    const int bd = hb.bd, bb = bd * bd;
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int idx = tid + NT * k;
      const bool ok = idx < cnt;
      const int e = (ok ? idx : 0) % bb;
      const int r = (int)(short)(tw[k] >> 16) + e / bd, c = (int)(short)(tw[k] & 0xffff) + e % bd;
      const T val = base[(int64_t)tblk[k] * bb + e];
      if (ok && r >= 0 && r < TILE && c >= 0 && c < TILE) {
        rc[k] = (r << 8) | c;
        v[k] = val;
      }
    }
  }
  __device__ __forceinline__ void load(const HBlk& hb, int b, int ti, int tj, int tid) {
    load_tables(hb, ti, tj, tid);
    load_values(hb, b, tid);
  }
  template <typename F>
  __device__ __forceinline__ void foreach(const HBlk& hb, int b, int tid, F&& f) const {
#pragma unroll
    for (int k = 0; k < NPRE; ++k)
      if (rc[k] >= 0) f(rc[k] >> 8, rc[k] & 255, v[k]);
    if (cnt > NT * NPRE) {   // a tile with more pieces than the registers hold
      const T* base = static_cast<const T*>(hb.blocks) + (int64_t)b * hb.bstride;
      const int bd = hb.bd, bb = bd * bd;
      if (bd == 6) {
        // ONE PIECE PER THREAD (6 x 6 blocks: the reduced camera system of a bundle adjustment fills a tile with up to 21 x 21
        // of them -- 15876 elements; element by element that was 62 rounds of  table, table, value  per thread): a block is 36
        // contiguous values, read as three batches of twelve (16-byte vectors), its table entries once.  The piece that holds
        // element 256 NPRE of the tile's run is split with the register part above.
        constexpr int VEC = 16 / sizeof(T), NV = 12 / VEC;
        typedef T TV __attribute__((ext_vector_type(VEC)));
        const int pb = (NT * NPRE) / 36, eb = (NT * NPRE) % 36, np = cnt / 36;
        for (int q = pb + tid; q < np; q += NT) {
          const int w = hb.piece_rc[p0 + q];
          const int r0 = (int)(short)(w >> 16), c0 = (int)(short)(w & 0xffff);
          const TV* src = reinterpret_cast<const TV*>(base + (int64_t)hb.piece_blk[p0 + q] * 36);
          const int e0 = q == pb ? eb : 0;
#pragma unroll
          for (int part = 0; part < 3; ++part) {
            TV val[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) val[k] = src[NV * part + k];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
              const int e = 12 * part + k;           // (compile-time: e / 6, e % 6 are constants)
              const int r = r0 + e / 6, c = c0 + e % 6;
              if (e >= e0 && r >= 0 && r < TILE && c >= 0 && c < TILE) f(r, c, val[k / VEC][k % VEC]);
            }
          }
        }
      } else {
        for (int idx = tid + NT * NPRE; idx < cnt; idx += NT) {
          const int pc = p0 + idx / bb, e = idx % bb;
          const int w = hb.piece_rc[pc];
          const int r = (int)(short)(w >> 16) + e / bd, c = (int)(short)(w & 0xffff) + e % bd;
          if (r >= 0 && r < TILE && c >= 0 && c < TILE) f(r, c, base[(int64_t)hb.piece_blk[pc] * bb + e]);
        }
      }
    }
  }
};
constexpr int HB_NPRE_OFF = 3;    // off-diagonal tiles of a pose graph: <= ~20 pieces (720 elements)

// The pieces of the ADJACENT lower tiles (ti, tj) and (ti, tj + 1) (chol_offdiag2: one workgroup produces both): their runs of
// the piece list are consecutive (tile index ti (ti + 1) / 2 + tj), so they are fetched as ONE run -- both tables of all
// elements in one batch, one exposed round trip, the values in flight until the first gather.  rc: (tile << 16) | (r << 8) | c.
template <typename T, int NPRE>
struct HBPre2 {
  T v[NPRE];
  int rc[NPRE];
  int p0, p1, cnt;   // first piece of tile 0 / of tile 1, elements of both
  int wmeta;         // (HBPre: lane l holds piece_rc of piece l of the run)
  __device__ __forceinline__ void to_list(T* list, int tid) const {
#pragma unroll
    for (int k = 0; k < NPRE; ++k)
      if (tid + 256 * k < cnt) list[tid + 256 * k] = v[k];   // (k < NPRE: what the registers hold)
  }
  int tw[NPRE], tblk[NPRE], tpc[NPRE];   // (HBPre: the two phases)
  __device__ __forceinline__ void load_tables(const HBlk& hb, int ti, int tj, int tid) {
    load_tables_run(hb, ti * (ti + 1) / 2 + tj, tid);
  }
  // (the runs t, t + 1 of whatever tile_ptr / piece_* tables ``hb`` carries: the row groups' tables are keyed by group)
  __device__ __forceinline__ void load_tables_run(const HBlk& hb, int t, int tid) {
    const int bd = hb.bd, bb = bd * bd;
    p0 = hb.tile_ptr[t];
    p1 = hb.tile_ptr[t + 1];
    cnt = (hb.tile_ptr[t + 2] - p0) * bb;
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      rc[k] = -1;
      v[k] = T(0);
      tw[k] = tblk[k] = tpc[k] = 0;
    }
    wmeta = 0;
    if (cnt <= 0) return;   // (workgroup uniform)
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int idx = tid + 256 * k;
      tpc[k] = p0 + (idx < cnt ? idx : 0) / bb;
      tw[k] = hb.piece_rc[tpc[k]];
      tblk[k] = hb.piece_blk[tpc[k]];
    }
    wmeta = hb.piece_rc[p0 + min(tid & 63, cnt / bb - 1)];
  }
  __device__ __forceinline__ void load_values(const HBlk& hb, int b, int tid) {
    if (cnt <= 0) return;
    const T* base = static_cast<const T*>(hb.blocks) + (int64_t)b * hb.bstride;
    const int bd = hb.bd, bb = bd * bd;
#pragma unroll
    for (int k = 0; k < NPRE; ++k) {
      const int idx = tid + 256 * k;
      const bool ok = idx < cnt;
      const int e = (ok ? idx : 0) % bb;
      const int r = (int)(short)(tw[k] >> 16) + e / bd, c = (int)(short)(tw[k] & 0xffff) + e % bd;
      const T val = base[(int64_t)tblk[k] * bb + e];
      if (ok && r >= 0 && r < TILE && c >= 0 && c < TILE) {
        rc[k] = ((tpc[k] >= p1 ? 1 : 0) << 16) | (r << 8) | c;
        v[k] = val;
      }
    }
  }
  __device__ __forceinline__ void load(const HBlk& hb, int b, int ti, int tj, int tid) {
    load_tables(hb, ti, tj, tid);
    load_values(hb, b, tid);
  }
  __device__ __forceinline__ void load_run(const HBlk& hb, int b, int t, int tid) {
    load_tables_run(hb, t, tid);
    load_values(hb, b, tid);
  }
  // f(r, c, value) for the pieces of tile ``sel`` (0 / 1)
  template <typename F>
  __device__ __forceinline__ void foreach(const HBlk& hb, int b, int tid, int sel, F&& f) const {
#pragma unroll
    for (int k = 0; k < NPRE; ++k)
      if (rc[k] >= 0 && (rc[k] >> 16) == sel) f((rc[k] >> 8) & 255, rc[k] & 255, v[k]);
    if (cnt > 256 * NPRE) {   // (rare: more pieces than the registers hold)
      const T* base = static_cast<const T*>(hb.blocks) + (int64_t)b * hb.bstride;
      const int bd = hb.bd, bb = bd * bd;
      for (int idx = tid + 256 * NPRE; idx < cnt; idx += 256) {
        const int pc = p0 + idx / bb, e = idx % bb;
        if ((pc >= p1 ? 1 : 0) != sel) continue;
        const int w = hb.piece_rc[pc];
        const int r = (int)(short)(w >> 16) + e / bd, c = (int)(short)(w & 0xffff) + e % bd;
        if (r >= 0 && r < TILE && c >= 0 && c < TILE) f(r, c, base[(int64_t)hb.piece_blk[pc] * bb + e]);
      }
    }
  }
};
constexpr int HB_NPRE_DIAG = 7;   // diagonal tiles: ~21 diagonal blocks + their chain / loop-closure neighbours (~49 pieces)

// ---- H_ij's pieces ADDED to the accumulators by the matrix cores (round 6) ----
// The gather rounds above (zero half a tile of LDS, scatter, barrier, read it back in the accumulator layout, barrier -- 2 rounds
// in fp32, 4 in fp64, 7 / 13 barriers) cost 17 k (fp32) / 40 k (fp64) cycles per tile while the partner workgroup is in its
// K-loop: 2.4 of 44 ms and 5.7 of 93 ms of the headline factorisations (profiles/r6: the same launches with a register-only fake
// of the gather).  A pose graph's off-diagonal tile holds <= ~20 blocks of 6 x 6: 720 values for 16384 accumulators.  So:
// P = -P in registers, the tile's values as ONE contiguous list in LDS (one barrier), and per piece a rank-bd update on the matrix
// cores, acc(tile column c, tile row r) += sum_k [c == c0 + k] V[r - r0][k]: operand A is a 0/1 selector computed from the lane
// index, operand B the piece's values of this lane's row, the accumulator block is picked by wave-uniform branches (the piece's
// origin comes from lane p of ``wmeta`` by readlane).  One exact product v * 1 per element, every other term 0 * x = 0: the result
// is the bit pattern of  v - sum  as before (up to the sign of a zero).
// fp32, v_mfma_f32_32x32x2: lane (rr = lane & 31, g = lane >> 5) supplies A[i = rr][k = g], B[k = g][j = rr]; acc.v[cb][v] is
// D[i = 8 (v / 4) + 4 g + v % 4][j = rr] = tile (row 32 wave + rr, column 32 cb + i)
__device__ __forceinline__ void hb_scatter(Engine<float>::Acc& P, const float* list, int wmeta, int pa, int pb, int bd, int wave,
                                           int lane) {
  const int rr = lane & 31, g = lane >> 5, bb = bd * bd, rw0 = 32 * wave;
  // lane l looks at piece l: does it touch this wave's rows / block cb's columns?  One ballot per accumulator block, then a loop
  // over the set bits -- every loop updates ONE accumulator block (one loop over the pieces with a branch per block made hipcc
  // shuffle the accumulators between registers and spill)
  const int r0l = (int)(short)(wmeta >> 16), c0l = (int)(short)(wmeta & 0xffff);
  const bool rowhit = lane >= pa && lane < pb && r0l + bd > rw0 && r0l < rw0 + 32;
  static_for<4>([&](auto icb) __attribute__((always_inline)) {
    constexpr int cb = decltype(icb)::value;
    unsigned long long mask = __builtin_amdgcn_ballot_w64(rowhit && c0l + bd > 32 * cb && c0l < 32 * cb + 32);
    while (mask) {
      const int p = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int w = __builtin_amdgcn_readlane(wmeta, p);
      const int r0 = (int)(short)(w >> 16), c0 = (int)(short)(w & 0xffff);
      const int dr = rw0 + rr - r0;
      const bool rin = dr >= 0 && dr < bd;
      const float* src = list + p * bb + (rin ? dr : 0) * bd;
      const int t = c0 + g - rr - 32 * cb;   // A[i = rr][k = g], step m: 32 cb + rr == c0 + 2 m + g
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const int kc = 2 * m + g;
        const float x = src[min(kc, bd - 1)];
        if (2 * m < bd)
          P.v[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(t + 2 * m == 0 ? 1.f : 0.f, rin && kc < bd ? x : 0.f, P.v[cb], 0, 0, 0);
      }
    }
  });
}
// fp64, v_mfma_f64_16x16x4: lane (rl = lane & 15, kq = lane >> 4) supplies A[i = rl][k = kq], B[k = kq][j = rl]; acc.v[h][cb][v] is
// D[i = 4 v + kq][j = rl] = tile (row 32 wave + 16 h + rl, column 16 cb + i)
__device__ __forceinline__ void hb_scatter(Engine<double>::Acc& P, const double* list, int wmeta, int pa, int pb, int bd, int wave,
                                           int lane) {
  const int rl = lane & 15, kq = lane >> 4, bb = bd * bd, rw0 = 32 * wave;
  const int r0l = (int)(short)(wmeta >> 16), c0l = (int)(short)(wmeta & 0xffff);
  const bool mine = lane >= pa && lane < pb;
  static_for<2>([&](auto ih) __attribute__((always_inline)) {
    constexpr int h = decltype(ih)::value;
    const int rh0 = rw0 + 16 * h;
    const bool rowhit = mine && r0l + bd > rh0 && r0l < rh0 + 16;
    static_for<8>([&](auto icb) __attribute__((always_inline)) {
      constexpr int cb = decltype(icb)::value;
      unsigned long long mask = __builtin_amdgcn_ballot_w64(rowhit && c0l + bd > 16 * cb && c0l < 16 * cb + 16);
      while (mask) {
        const int p = __builtin_ctzll(mask);
        mask &= mask - 1;
        const int w = __builtin_amdgcn_readlane(wmeta, p);
        const int r0 = (int)(short)(w >> 16), c0 = (int)(short)(w & 0xffff);
        const int dr = rh0 + rl - r0;
        const bool rin = dr >= 0 && dr < bd;
        const double* src = list + p * bb + (rin ? dr : 0) * bd;
        const int t = c0 + kq - rl - 16 * cb;   // A[i = rl][k = kq], step m: 16 cb + rl == c0 + 4 m + kq
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const int kc = 4 * m + kq;
          const double x = src[min(kc, bd - 1)];
          if (4 * m < bd)
            P.v[h][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(t + 4 * m == 0 ? 1.0 : 0.0, rin && kc < bd ? x : 0.0, P.v[h][cb], 0, 0, 0);
        }
      }
    });
  });
}

// (the 8-wave fp64 off-diagonal kernel: a wave owns 16 rows of the tile -- acc.v[cb][v] = tile (row 16 wave + rl, column 16 cb + 4 v + kq))
struct Acc16 {
  f64x4 v[8];
};
__device__ __forceinline__ void hb_scatter(Acc16& P, const double* list, int wmeta, int pa, int pb, int bd, int wave, int lane) {
  const int rl = lane & 15, kq = lane >> 4, bb = bd * bd, rh0 = 16 * wave;
  const int r0l = (int)(short)(wmeta >> 16), c0l = (int)(short)(wmeta & 0xffff);
  const bool rowhit = lane >= pa && lane < pb && r0l + bd > rh0 && r0l < rh0 + 16;
  static_for<8>([&](auto icb) __attribute__((always_inline)) {
    constexpr int cb = decltype(icb)::value;
    unsigned long long mask = __builtin_amdgcn_ballot_w64(rowhit && c0l + bd > 16 * cb && c0l < 16 * cb + 16);
    while (mask) {
      const int p = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int w = __builtin_amdgcn_readlane(wmeta, p);
      const int r0 = (int)(short)(w >> 16), c0 = (int)(short)(w & 0xffff);
      const int dr = rh0 + rl - r0;
      const bool rin = dr >= 0 && dr < bd;
      const double* src = list + p * bb + (rin ? dr : 0) * bd;
      const int t = c0 + kq - rl - 16 * cb;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int kc = 4 * m + kq;
        const double x = src[min(kc, bd - 1)];
        if (4 * m < bd)
          P.v[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(t + 4 * m == 0 ? 1.0 : 0.0, rin && kc < bd ? x : 0.0, P.v[cb], 0, 0, 0);
      }
    }
  });
}

// acc += the pieces [lo, hi) of the run ``pre`` describes (HBPre: the tile's, HBPre2: both tiles').  Chunk 0 -- the pieces that sit in
// the registers whole, at most 64 (wmeta) -- goes through ``list`` (written here when ``write_list``: once per run, the caller
// guarantees the buffer is free); a tile with more pieces (rare in a pose graph: > 21 blocks of 6 x 6 in one 128 x 128 tile) takes
// further chunks of 64 straight from memory into ``list + LIST0`` -- two dependent loads and two barriers each, exposed.
// Workgroup uniform control flow; LDS use: LIST0 + 64 bd^2 elements.
constexpr int HB_MODE_SCATTER = 1, HB_MODE_ROUNDS = 2;   // the kernels' HB template argument (0: dense H)
template <typename T, typename Acc, typename Pre, int LIST0, int NT = 256>
__device__ __forceinline__ void hb_add(Acc& P, const Pre& pre, const HBlk& hb, int b, T* list, int lo, int hi, bool write_list,
                                       int tid) {
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int bd = hb.bd, bb = bd * bd;
  const int nreg = min(min(pre.cnt / bb, LIST0 / bb), 64);
  if (write_list) {
    pre.to_list(list, tid);
    __syncthreads();
  }
  hb_scatter(P, list, pre.wmeta, lo, min(hi, nreg), bd, wave, lane);
  if (hi > nreg) {   // (workgroup uniform)
    const T* base = static_cast<const T*>(hb.blocks) + (int64_t)b * hb.bstride;
    T* over = list + LIST0;
    for (int q0 = max(lo, nreg); q0 < hi; q0 += 64) {
      const int nq = min(64, hi - q0);
      __syncthreads();   // the previous chunk has been read
      for (int idx = tid; idx < nq * bb; idx += NT) over[idx] = base[(int64_t)hb.piece_blk[pre.p0 + q0 + idx / bb] * bb + idx % bb];
      const int wm = hb.piece_rc[pre.p0 + q0 + min(lane, nq - 1)];
      __syncthreads();
      hb_scatter(P, over, wm, 0, nq, bd, wave, lane);
    }
  }
}

}  // namespace thx
