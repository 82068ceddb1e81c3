// Batched damped dense Cholesky (factor + solves) for gfx950, one problem per workgroup-chain.
//
// Replaces DenseSolver._apply_damping + CholeskyDenseSolver._solve_sytem
// (theseus/optimizer/linear/dense_solver.py:38-64,159-161) for a batch of B SPD matrices of order n.
//
// Algorithm: tiled LEFT-LOOKING Cholesky with 128x128 tiles, one kernel launch pair per block
// column j (the batch supplies the parallelism: B x (N-j) workgroups per launch, no inter-workgroup
// communication inside a launch):
//   chol_diag(j)    : S = H_jj + damping - L_j,0:j L_j,0:j^T   (MFMA K-loop; the same pass over the
//                     panel also forms L_j,0:j y_0:j for the fused forward substitution)
//                     L_jj = chol(S)                            (register-resident, row per lane pair)
//                     panel M_j: 32x32 diagonal sub-blocks W_ss = L_ss^-1 (inverted in fp64), strictly
//                     lower sub-blocks -L_st;  y_j = L_jj^-1 (g_j - L_j,0:j y)  (blocked, via M_j)
//   chol_offdiag(j) : P = H_ij - L_i,0:j L_j,0:j^T              (MFMA K-loop)
//                     L_ij = P L_jj^-T as a BLOCKED substitution on the matrix cores:
//                       for s = 0..3:  P_s += sum_{t<s} X_t (-L_st)^T ;  X_s = P_s W_ss^T
//                     The accumulator registers are fed straight back as the MFMA B operand (the
//                     k index of an MFMA is just a pairing of columns, and the pairing the C/D
//                     layout gives is as good as any), A comes from the panel in LDS: no data
//                     movement, 160 MFMAs per wave instead of 128 dependent VALU/LDS steps.
// Left-looking means every tile of L is written exactly once and the trailing matrix is never
// re-read: per problem the K-loops stream  sum_j (N-j) * 2*128*(128 j)  elements.
// Only 32x32 triangles are ever inverted (in fp64, rounded once): the substitution across sub-blocks
// uses L itself, so the result has the error profile of a blocked TRSM, not of a full inverse.
//
// MFMA mapping (f32: v_mfma_f32_32x32x2_f32, f64: v_mfma_f64_16x16x4_f64): a 256-thread workgroup is
// 4 waves; wave w owns tile rows [32w, 32w+32) x all 128 columns and computes the TRANSPOSED product
// block D = L_j-rows * L_i-rows^T, so that a lane holds ONE matrix row (f32: row 32w + (lane&31),
// columns with ((c>>2)&1) == lane>>5; f64: row 32w + 16h + (lane&15), columns c = lane>>4 mod 4).
//
// Solves: L y = g is fused into the factorisation (above); L^T x = y is one HBM-bound pass over L
// (chol_bwd_kernel).  A stand-alone forward kernel serves solves with a cached factor (implicit
// backward pass).
#include "common.cuh"
#include "chol_base.cuh"
#include "chol_engine.cuh"
#include "chol_potrf.cuh"
#include "chol_tiles.cuh"
#include "chol_diag.cuh"
#include "chol_offdiag_f32.cuh"
#include "chol_offdiag_f64.cuh"
#include "chol_solve.cuh"
#include "chol_small.cuh"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

namespace thx {

constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr int FACTOR_NEEDS_FORWARD = 1000;   // factor_impl -> factor_then_forward: factor done, y = L^-1 rhs still to be computed
constexpr int BWD_ROWS_MAX_BATCH = 32;       // solve_impl: the backward substitution block row by block row up to this batch

// Defaults of the per-call schedule (thx_chol_schedule; a negative field / a NULL pointer selects them).  The library keeps no
// mutable schedule state: two callers with different schedules in one process do not see each other.
constexpr int SPLIT_DIAG_MIN_DEFAULT = 2048;
constexpr int COLUMN_PAIRS_DEFAULT = 1;

// Launch-side state is kept PER DEVICE (a process may drive several GPUs, from several threads): the auxiliary stream + events of
// the two-stream schedules, which belong to the device they were created on, and the dynamic-LDS limits (launch_lds).
constexpr int MAX_DEVICES = 64;
struct DeviceLaunchState {
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_lag = nullptr, ev_join = nullptr;
  hipEvent_t ev_diag = nullptr, ev_rest = nullptr;   // look-ahead schedule (one part): diag(j) done / rest of column j done
  // the auxiliary stream and the events of the two-stream schedules, created on first use
  void need_aux() {
    if (aux) return;
    hipStreamCreateWithFlags(&aux, hipStreamNonBlocking);
    for (hipEvent_t* e : {&ev_fork, &ev_lag, &ev_join, &ev_diag, &ev_rest}) hipEventCreateWithFlags(e, hipEventDisableTiming);
  }
};
static std::mutex g_launch_mutex;
static int current_device() {
  int dev = 0;
  hipGetDevice(&dev);
  return (dev >= 0 && dev < MAX_DEVICES) ? dev : 0;
}
static DeviceLaunchState& launch_state(int dev) {
  static DeviceLaunchState st[MAX_DEVICES];
  return st[dev];
}

// Launches Kernel with `smem` bytes of dynamic LDS, first raising the kernel's limit on device `dev` (current_device()) if it does
// not stand that high yet: remembered per kernel instance (one instance of this template each) and per device, so a kernel cannot
// be launched without its limit.  Only under g_launch_mutex.
template <auto Kernel, typename... A>
static void launch_lds(int dev, dim3 grid, dim3 block, size_t smem, hipStream_t s, A... args) {
  static size_t have[MAX_DEVICES] = {};
  if (smem > have[dev]) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    have[dev] = smem;
  }
  hipLaunchKernelGGL(Kernel, grid, block, smem, s, args...);
}

// a run-time value as a template argument: f(std::integral_constant<...>{})
template <typename F>
static void with_bool(bool b, F&& f) {
  b ? f(std::true_type{}) : f(std::false_type{});
}
template <typename F>
static void with_hb_mode(int hbm, F&& f) {   // (FactorPlan.hbm: the off-diagonal kernels' HB template argument)
  if (hbm == 0) f(std::integral_constant<int, 0>{});
  else if (hbm == HB_MODE_SCATTER) f(std::integral_constant<int, HB_MODE_SCATTER>{});
  else f(std::integral_constant<int, HB_MODE_ROUNDS>{});
}

// how an off-diagonal tile takes its pieces of H: a few per tile (pose graphs) -> added by the matrix cores (hb_scatter); many (a
// bundle adjustment's reduced camera system: up to 21 x 21 blocks per tile) or unknown -> gathered through LDS in rounds
constexpr int HB_SCATTER_MAX_PIECES_DEFAULT = 64;
// fp64: the first f64_wide_max block columns (K-loops shorter than that many tiles) take the 8-wave off-diagonal kernel
// (chol_offdiag_f64w8_kernel).  Default: ALL of them -- measured +1.0 ... 1.3 % at batch 256 / 1024 / 4096 (n = 1536), growing with
// the number of columns that use it (profiles/r6/ae_): four waves per SIMD serve the K-loop better than two; the early columns,
// for which the kernel was written, gain nothing.
constexpr int F64_WIDE_MAX_KTILES_DEFAULT = 1 << 30;
// ... and the first f64_half_max of them (K-loops shorter than that many tiles) the HALF-TILE kernel (chol_offdiag_f64h_kernel, four
// workgroups per CU): measured optimum 6 ... 8 at n = 1536 / batch 4096 (profiles/r6/af_: 90.0 -> 88.5 ms; all twelve columns 89.0)
constexpr int F64_HALF_MAX_KTILES_DEFAULT = 8;
// batch size from which the batch is dealt over two streams (factor_impl)
constexpr int SPLIT_MIN = 1024;
// (pairs from 128 problems per call on: the pair schedule's chain per two columns is diag, head tile, diag, pair tiles -- one
//  more dependent launch than two plain columns -- and below ~128 problems the launches are too small to pay for it: n = 1536,
//  batch 8 / 16 / 32 / 64: 1.62 / 1.64 / 1.67 / 1.85 ms with pairs, 1.42 / 1.44 / 1.50 / 1.73 ms without; 128: 2.25 / 2.23; 256:
//  3.25 / 3.30 -- profiles/r6/j_ab_small_batch.txt.  Bit-identical either way.)
constexpr int COLUMN_PAIRS_MIN_BATCH_DEFAULT = 128;

// THE LAUNCH PLAN of a factorisation: every schedule decision factor_impl takes from its arguments, the per-call schedule and the
// defaults above -- in one place, so that thx_chol_plan reports exactly what a call with those arguments runs.
enum class Schedule { Levels, LookAhead, RightLooking, LeftLooking };   // run_levels, run_lookahead, run_right_looking, run_left_looking
struct FactorPlan {
  Schedule schedule;
  int ntiles;
  int split_diag_min;    // (the level schedule decides per level with it)
  bool fused_diag;       // the diagonal phase as one kernel (else SYRK + potrf)
  int rl_max_batch;
  bool split;            // (left-looking) the batch dealt over two streams
  int nparts;            // 2 if split, else 1
  int rl_mode;           // (right-looking) its launch arrangement (0 | 1 | 2)
  bool rl_fwd_fused;     // ... with the forward substitution riding on it (else FACTOR_NEEDS_FORWARD)
  bool colpair;          // (left-looking) the column-pair schedule (fp32)
  bool zskip;            // the off-diagonal K-loops skip structurally zero 32x32 sub-blocks (HBlk.l_mask; fp32 left-looking dense frame)
  bool regroup;          // ... and the column pairs that have row groups take them (HBlk.rg_*, thx_chol_schedule.regroup_rows)
  bool zsolve;           // ... their waves skip zero solves (HBlk.rg_zf) and / or pair 0 runs on groups (thx_chol_schedule.skip_zero_solves)
  bool pair0;            // pair 0 takes its own row groups (HBlk.rg0_*; only with zsolve)
  bool sortcols;         // the pairs with row groups and sorted-column tables take those too (HBlk.sc_*, thx_chol_schedule.sort_pair_columns)
  bool sorthead;         // the pairs' head tiles (j + 1, j) whose tile j has sorted-column tables take them (HBlk.th_*, thx_chol_schedule.sort_tile_rows)
  bool sortrows;         // the split diagonal phase's SYRK stages the tiles that have sorted-row tables by them (HBlk.tr_*, thx_chol_schedule.sort_tile_rows)
  int hbm;               // the off-diagonal kernels' HB template argument: 0 dense H, HB_MODE_SCATTER, HB_MODE_ROUNDS
  int f64_wide_max, f64_half_max;
};

static FactorPlan plan_factor(bool f64, int n, int64_t ld, int B, bool has_damping, bool has_rhs, int64_t ldv, bool y_aligned16,
                              const thx_tile_pattern* tp, const HBlk* hbp, const thx_level_schedule* ls, const thx_chol_schedule* sched) {
  FactorPlan p{};
  const bool use_hb = hbp != nullptr;
  const bool packed = ld == 0;
  p.ntiles = (n + TILE - 1) / TILE;
  const int hb_scatter_max = (sched && sched->hb_scatter_max_pieces >= 0) ? sched->hb_scatter_max_pieces : HB_SCATTER_MAX_PIECES_DEFAULT;
  const bool hb_sc = use_hb && hbp->bd <= 6 && hbp->max_tile_pieces > 0 && hbp->max_tile_pieces <= hb_scatter_max;
  p.hbm = !use_hb ? 0 : (hb_sc ? HB_MODE_SCATTER : HB_MODE_ROUNDS);
  p.f64_wide_max = (sched && sched->f64_wide_max_ktiles >= 0) ? sched->f64_wide_max_ktiles : F64_WIDE_MAX_KTILES_DEFAULT;
  p.f64_half_max = (sched && sched->f64_half_max_ktiles >= 0) ? sched->f64_half_max_ktiles : F64_HALF_MAX_KTILES_DEFAULT;
  // diagonal phase: chol_syrk_kernel + chol_potrf_kernel from split_diag_min problems per call on (measured, n = 1536: fp32
  // 45.1 vs 46.0 ms at batch 4096, fp64 101.6 vs 105.2 ms; equal at batch 1024; 3.74 vs 3.51 ms at batch 256 -- the second
  // launch per column costs more than the chain there), else the fused chol_diag_kernel
  p.split_diag_min = (sched && sched->split_diag_min_batch >= 0) ? sched->split_diag_min_batch : SPLIT_DIAG_MIN_DEFAULT;
  const int column_pairs = (sched && sched->column_pairs >= 0) ? sched->column_pairs : COLUMN_PAIRS_DEFAULT;
  const int pair_min_batch =
      (sched && sched->column_pairs_min_batch >= 0) ? sched->column_pairs_min_batch : COLUMN_PAIRS_MIN_BATCH_DEFAULT;
  // (default hand-over to the left-looking schedule, measured at 12 block columns with two launches per column, profiles/r6/ar_:
  //  fp32 right-looking wins through 64 problems -- batch 40 1.49 -> 1.16 ms, 64 1.66 -> 1.58 --, fp64 through 40; the update
  //  launches grow with the SQUARE of the block columns, so the limit shrinks with them, down to round 6's first 32)
  const int rl_auto = !f64 ? min(64, max(32, 768 / max(p.ntiles, 1))) : min(40, max(32, 480 / max(p.ntiles, 1)));
  p.rl_max_batch = (sched && sched->right_looking_max_batch >= 0) ? sched->right_looking_max_batch : rl_auto;
  p.fused_diag = B < p.split_diag_min;
  p.split = B >= SPLIT_MIN && p.ntiles > 1;
  p.nparts = p.split ? 2 : 1;
  p.schedule = Schedule::Levels;
  if (ls) return p;   // (its own launch loop, per level)
  p.schedule = Schedule::LookAhead;
  if (!p.split && p.ntiles > 2 && tp && tp->col_head_host != nullptr) return p;
  p.schedule = Schedule::RightLooking;
  if (!tp && !packed && !p.split && p.fused_diag && p.ntiles >= 3 && B <= p.rl_max_batch && ld >= (int64_t)p.ntiles * TILE &&
      (!use_hb || !has_damping || hbp->diag_blk)) {
    const int m = sched ? sched->right_looking_mode : -1;
    p.rl_mode = m < 0 ? (f64 ? 2 : 1) : (m > 2 ? 1 : m);
    p.rl_fwd_fused = has_rhs && (ldv % 4) == 0 && y_aligned16;
    return p;
  }
  p.schedule = Schedule::LeftLooking;
  p.colpair = column_pairs != 0 && !f64 && !tp && !packed && B >= pair_min_batch;
  p.zskip = !f64 && !tp && !packed && use_hb && hbp->l_mask != nullptr && (!sched || sched->skip_zero_blocks != 0);
  // row groups: the pair kernel only, a layout that carries all the tables, every group's pieces within what the matrix-core
  // scatter is allowed per tile, and row offsets anywhere in the frame that fit the buffer loads' 32-bit offsets
  p.regroup = p.zskip && p.colpair && (!sched || sched->regroup_rows != 0) && hbp->rg_group_ptr_host && hbp->rg_rows && hbp->rg_k0 &&
              hbp->rg_tile_ptr && hbp->rg_piece_blk && hbp->rg_piece_rc &&
              (p.hbm != HB_MODE_SCATTER || hbp->rg_max_tile_pieces <= hb_scatter_max) && (int64_t)n * ld * 4 < ((int64_t)1 << 31);
  // zero solves: wherever regrouping may apply -- the groups' per-wave first chunks, and pair 0 on groups of its own (a layout may have
  // these without any group above: three block columns).  Pair 0 alone falls back to natural tiles over the scatter limit.
  const bool zs = p.zskip && p.colpair && (!sched || (sched->regroup_rows != 0 && sched->skip_zero_solves != 0)) &&
                  (int64_t)n * ld * 4 < ((int64_t)1 << 31);
  p.pair0 = zs && p.ntiles > 2 && hbp->rg0_ngroups > 0 && hbp->rg0_rows && hbp->rg0_zf && hbp->rg0_tile_ptr && hbp->rg0_piece_blk &&
            hbp->rg0_piece_rc && (p.hbm != HB_MODE_SCATTER || hbp->rg0_max_tile_pieces <= hb_scatter_max);
  p.zsolve = (zs && p.regroup && hbp->rg_zf) || p.pair0;
  p.sortcols = p.regroup && (!sched || sched->sort_pair_columns != 0) && hbp->sc_pair_host && hbp->sc_perm && hbp->sc_mask;
  p.sorthead = p.regroup && p.hbm != 0 && (!sched || sched->sort_tile_rows != 0) && hbp->th_tile_host && hbp->th_perm32 && hbp->th_mask32 &&
               hbp->th_k0h;
  p.sortrows = p.regroup && !p.fused_diag && (!sched || sched->sort_tile_rows != 0) && hbp->tr_tile_host && hbp->tr_perm16 && hbp->tr_mask16;
  return p;
}

struct Half { hipStream_t s; int b0, nb; };   // some of the batch on one stream: problems [b0, b0 + nb)

// ONE FACTORISATION BEING ENQUEUED: the call's arguments, its plan and what every schedule derives from them, with the launches
// the schedules share as members.  Built by factor_impl under g_launch_mutex; the four run_* functions below hold the schedules.
template <typename T>
struct FactorLaunch {
  const void* H; int64_t ld; int n, B; const void* damping; int ellipsoidal; double eps;   // (factor_impl's arguments)
  void* L; void* panel; int32_t* info; const void* rhs; void* y; int64_t ldv; hipStream_t st;
  const thx_tile_pattern* tp; const thx_level_schedule* ls;
  FactorPlan P;
  TilePat pat;
  bool use_hb;
  HBlk hb;                    // (l_mask only with P.zskip: under every other schedule, and with skipping switched off, the kernels see no mask)
  bool packed;                // ld == 0: L is the TILE-PACKED factor (B, nslots, TILE, TILE) of the pattern
  int64_t hstride, lstride;   // elements per problem: the H frame (dense H only; never packed), L
  size_t dsm;                 // dynamic LDS of the diagonal phase P.fused_diag selects, with the whole y buffer if there is a rhs
  int dev; DeviceLaunchState& ds;   // current_device() and its launch_state

  // the half's first problem in L, in the panels and in the dense H frame (block-compact H: the half's problems start at h.b0 of the
  // block list; H itself is not dereferenced)
  T* L_of(const Half& h) const { return (T*)L + (int64_t)h.b0 * lstride; }
  T* panel_of(const Half& h) const { return (T*)panel + (int64_t)h.b0 * P.ntiles * TILE * TILE; }
  const T* H_of(const Half& h) const { return use_hb ? nullptr : (const T*)H + (int64_t)h.b0 * hstride; }
  HBlk hb_of(const Half& h) const {
    HBlk x = hb;
    if (use_hb) x.blocks = static_cast<const T*>(hb.blocks) + (int64_t)h.b0 * hb.bstride;
    return x;
  }

  // row tiles [i_first, i_first + nrt) of block column j (tile-sparse / levels: entries of the pattern), one workgroup each
  void off(const Half& h, int j, int i_first, int nrt) const {
    const int ntiles = P.ntiles, Bpad = (h.nb + 7) / 8 * 8;
    with_hb_mode(P.hbm, [&](auto mode) {
      constexpr int M = decltype(mode)::value;
      if constexpr (sizeof(T) == 4) {
        launch_lds<chol_offdiag_f32_kernel<M>>(dev, dim3(Bpad * nrt), dim3(256), OFF32_SMEM, h.s, H_of(h), L_of(h), panel_of(h), n, ld, j,
                                               ntiles, i_first, nrt, h.nb, pat, hb_of(h));
      } else {
        if constexpr (M != HB_MODE_ROUNDS) {
          if (!tp && !packed && j < P.f64_half_max) {   // (half tiles, four workgroups per CU, for the short K-loops)
            launch_lds<chol_offdiag_f64h_kernel<M>>(dev, dim3(Bpad * nrt * 2), dim3(256), OFF64_STAGE, h.s, H_of(h), L_of(h), panel_of(h),
                                                    n, ld, j, ntiles, i_first, nrt, h.nb, pat, hb_of(h));
            return;
          }
          if (!tp && j < P.f64_wide_max) {   // (dense schedule: column j's K-loops are j tiles long)
            launch_lds<chol_offdiag_f64w8_kernel<M>>(dev, dim3(Bpad * nrt), dim3(512), OFF64_SMEM, h.s, H_of(h), L_of(h), panel_of(h), n,
                                                     ld, j, ntiles, i_first, nrt, h.nb, pat, hb_of(h));
            return;
          }
        }
        launch_lds<chol_offdiag_f64_kernel<M>>(dev, dim3(Bpad * nrt), dim3(256), OFF64_SMEM, h.s, H_of(h), L_of(h), panel_of(h), n, ld, j,
                                               ntiles, i_first, nrt, h.nb, pat, hb_of(h));
      }
    });
  }

  // the head tile (j + 1, j) of column pair j: with sorted columns where tile j has a table (P.sorthead), else as any tile of column j
  void head(const Half& h, int j) const {
    if constexpr (sizeof(T) == 4) {
      if (P.sorthead && hb.th_tile_host[j]) {
        with_hb_mode(P.hbm, [&](auto mode) {
          constexpr int M = decltype(mode)::value;
          if constexpr (M != 0)
            launch_lds<chol_offdiag_f32_kernel<M, true>>(dev, dim3((h.nb + 7) / 8 * 8), dim3(256), OFF32_SMEM, h.s, H_of(h), L_of(h), panel_of(h),
                                                         n, ld, j, P.ntiles, j + 1, 1, h.nb, pat, hb_of(h));
        });
        return;
      }
    }
    off(h, j, j + 1, 1);
  }

  // tiles (i, j) and (i, j + 1) of row tiles [i_first, i_first + nrt) in one workgroup each (chol_offdiag2_f32_kernel)
  void pair(const Half& h, int j, int i_first, int nrt) const {
    if constexpr (sizeof(T) == 4)
      with_hb_mode(P.hbm, [&](auto mode) {
        launch_lds<chol_offdiag2_f32_kernel<decltype(mode)::value>>(dev, dim3((h.nb + 7) / 8 * 8 * nrt), dim3(256), OFF2_SMEM, h.s, H_of(h),
                                                                    L_of(h), panel_of(h), n, ld, j, P.ntiles, i_first, nrt, h.nb, hb_of(h));
      });
  }
  // ... of the row groups [g_first, g_first + ng) of pair j (P.regroup)
  void pair_groups(const Half& h, int j, int g_first, int ng) const { pair_groups(h, j, g_first, ng, hb_of(h)); }
  void pair_groups(const Half& h, int j, int g_first, int ng, const HBlk& x) const {
    if constexpr (sizeof(T) == 4)
      with_hb_mode(P.hbm, [&](auto mode) {
        constexpr int M = decltype(mode)::value;
        if constexpr (M != 0) {
          if (P.sortcols && j >= 2 && x.sc_pair_host[j / 2]) {   // this pair's sorted columns
            HBlk xs = x;
            xs.sc_perm = x.sc_perm + (int64_t)(j / 2) * 2 * TILE;
            xs.sc_mask = x.sc_mask + (int64_t)(j / 2) * 4 * P.ntiles;
            launch_lds<chol_offdiag2_f32_kernel<M, true, true>>(dev, dim3((h.nb + 7) / 8 * 8 * ng), dim3(256), OFF2_SMEM, h.s, H_of(h),
                                                                L_of(h), panel_of(h), n, ld, j, P.ntiles, g_first, ng, h.nb, xs);
            return;
          }
          launch_lds<chol_offdiag2_f32_kernel<M, true>>(dev, dim3((h.nb + 7) / 8 * 8 * ng), dim3(256), OFF2_SMEM, h.s, H_of(h), L_of(h),
                                                        panel_of(h), n, ld, j, P.ntiles, g_first, ng, h.nb, x);
        }
      });
  }

  // ... of pair 0's own groups (P.pair0): the same kernel, the rg_ tables of this launch are pair 0's
  void pair_groups0(const Half& h) const {
    HBlk x = hb_of(h);
    x.rg_rows = x.rg0_rows, x.rg_zf = x.rg0_zf, x.rg_tile_ptr = x.rg0_tile_ptr, x.rg_piece_blk = x.rg0_piece_blk, x.rg_piece_rc = x.rg0_piece_rc;
    x.rg_k0 = nullptr;   // (no K-loop)
    pair_groups(h, 0, 0, x.rg0_ngroups, x);
  }

  // the diagonal phase of block column j (nc > 1: the level schedule -- block columns [j, j + nc) in one launch, blockIdx.y the
  // column; `fused` / `smem`: which of the two diagonal schedules this launch takes, see FactorPlan.fused_diag)
  void diag(const Half& h, int j, int nc, bool fused, size_t smem) const {
    const int ntiles = P.ntiles;
    const T* rh = rhs ? (const T*)rhs + (int64_t)h.b0 * ldv : nullptr;
    T* yh = y ? (T*)y + (int64_t)h.b0 * ldv : nullptr;
    const T* dh = damping ? (const T*)damping + h.b0 : nullptr;
    with_bool(use_hb, [&](auto hbk) {
      constexpr bool HB = decltype(hbk)::value;
      if (fused)
        launch_lds<chol_diag_kernel<T, HB>>(dev, dim3(h.nb, nc), dim3(256), smem, h.s, H_of(h), L_of(h), panel_of(h), dh, ellipsoidal, (T)eps,
                                            info + h.b0, n, ld, j, ntiles, rh, yh, ldv, pat, hb_of(h));
      else {
        if constexpr (sizeof(T) == 4 && HB) {
          if (P.sortrows && nc == 1 && hb.tr_tile_host[j]) {   // this tile's sorted rows; the un-permute buffer lies over staging + y
            launch_lds<chol_syrk_kernel<T, HB, true>>(dev, dim3(h.nb, 1), dim3(256), std::max(smem, (size_t)SYRK_SR_TRI * sizeof(T)), h.s,
                                                      H_of(h), L_of(h), dh, ellipsoidal, (T)eps, n, ld, j, rh, yh, ldv, pat, hb_of(h));
            return;
          }
        }
        launch_lds<chol_syrk_kernel<T, HB>>(dev, dim3(h.nb, nc), dim3(256), smem, h.s, H_of(h), L_of(h), dh, ellipsoidal, (T)eps, n, ld, j, rh,
                                            yh, ldv, pat, hb_of(h));
      }
    });
    if (!fused) {
      const int64_t tile_off = packed ? (int64_t)j * TILE * TILE : (int64_t)j * TILE * ld + (int64_t)j * TILE;
      hipLaunchKernelGGL(chol_potrf_kernel<T>, dim3(h.nb, nc), dim3(64), 0, h.s, L_of(h), panel_of(h), info + h.b0, n, lstride,
                         tile_off, packed ? (int64_t)TILE : ld, j, ntiles, rh ? yh : nullptr, ldv, pat.tile_valid);
    }
  }
  void diag(const Half& h, int j) const { diag(h, j, 1, P.fused_diag, dsm); }
};

// LEVEL SCHEDULE (thx_chol_factor_levels): the block columns of one elimination-tree level do not depend on each other (a column
// needs, of the earlier columns, only those in which its own row panel is non-zero: its descendants in the tree) and the host
// numbered the columns level by level -- so: ONE diagonal launch and ONE off-diagonal launch per level, B x (columns of the
// level) and B x (entries of the level) workgroups.  A banded ordering's chain of ntiles dependent launch pairs becomes
// ~log2(ntiles) of them under a nested-dissection ordering (theseus_amd/sparse.py:LevelPattern).
template <typename T>
static int run_levels(const FactorLaunch<T>& c) {
  const thx_level_schedule* ls = c.ls;
  const Half h{c.st, 0, c.B};
  for (int l = 0; l < ls->nlevels; ++l) {
    const int j0 = ls->level_col_host[l], nc = ls->level_col_host[l + 1] - j0;
    const int e0 = ls->level_ent_host[l], ne = ls->level_ent_host[l + 1] - e0;
    if (nc <= 0) continue;
    // with the fused forward substitution a column keeps only its K-list's blocks of y in LDS: the launch of level l is sized for
    // the longest K-list of that level (level_maxk_host)
    const int yp = c.rhs ? ls->level_maxk_host[l] * TILE : 0;
    const bool fused = (int64_t)c.B * nc < c.P.split_diag_min;   // (both diagonal schedules may be taken, level by level)
    c.diag(h, j0, nc, fused, fused ? DiagSmem<T>::bytes(yp) : SyrkSmem<T>::bytes(yp));
    if (ne > 0) c.off(h, j0, e0, ne);
  }
  return check_launch("thx_chol_factor_levels");
}

// LOOK-AHEAD for batches that do not fill the chip (one part, i.e. B < SPLIT_MIN).
// Left-looking: tile (i, j) needs rows i and j of the columns before j.  So the diagonal phase of column j + 1 needs, of column
// j, only tile (j + 1, j) -- and at batch 256 that phase is B workgroups with one busy wave each (80 us on a 3072-column banded
// system, 24 times).  Column j's off-diagonal launch is therefore split: HEAD = tile (j + 1, j) on the caller's stream, followed
// at once by diag(j + 1); REST = the other row tiles on the auxiliary stream, concurrent with both.  Dependencies:
//   REST(j)  after diag(j)                     (event ev_diag; the earlier HEADs precede diag(j) on the caller's stream)
//   HEAD(j)  after diag(j) and REST(j - 1)     (row j + 1 of column j - 1 is a REST tile: event ev_rest)
//   diag(j+1) after HEAD(j) [stream order] -- its other inputs, rows j + 1 of columns < j, were waited for by HEAD(j).
// Tile-sparse: only if the host put tile (j + 1, j) FIRST in column j's entry list (col_head_host); otherwise the column runs
// as before (diag(j + 1) waits for all of column j).  Same kernels, same arithmetic: bit-identical results.
// Measured (profiles/r4/c_ab_lookahead_small_batch_factor.txt, same box, two rounds): the banded reduced camera system of the
// bundle-adjustment config (3072 columns, batch 256, 158 of 300 tiles) 6.82 -> 6.60 ms; DENSE frames do not gain (n = 1536:
// batch 256 3.5 ms either way, batch 512 6.2 -> 6.4 ms; n = 3072 batch 256 21.6 -> 21.8 ms: REST(j) of a dense column is most
// of the launch, the dispatcher does not run the two queues side by side) -- so: tile-sparse only.  (Nor between the right-looking
// schedule's batches and 256 problems, profiles/r6/ai_: batch 64 1.66 -> 1.88 ms, 128 2.18 -> 2.22, 256 3.16 -> 3.27 -- the
// whole off-diagonal launch is one round of workgroups there, HEAD(j) alone takes as long.)
template <typename T>
static int run_lookahead(const FactorLaunch<T>& c) {
  const thx_tile_pattern* tp = c.tp;
  DeviceLaunchState& ds = c.ds;
  ds.need_aux();
  const Half h0{c.st, 0, c.B}, h1{ds.aux, 0, c.B};
  hipEventRecord(ds.ev_fork, c.st);
  hipStreamWaitEvent(h1.s, ds.ev_fork, 0);
  bool rest_pending = false;   // a REST launch whose completion the caller's stream has not waited for yet
  for (int j = 0; j < c.P.ntiles; ++j) {
    c.diag(h0, j);
    const int nrt = tp->col_count_host[j];
    if (nrt <= 0) continue;
    const bool head = tp->col_head_host[j] != 0;   // the launch's first tile is (j + 1, j)
    const int n_head = head ? 1 : 0, n_rest = nrt - n_head;
    if (n_rest > 0) {
      hipEventRecord(ds.ev_diag, h0.s);
      hipStreamWaitEvent(h1.s, ds.ev_diag, 0);
    }
    if (rest_pending) {   // HEAD(j) / the next diagonal phase read REST(j - 1)'s tiles
      hipStreamWaitEvent(h0.s, ds.ev_rest, 0);
      rest_pending = false;
    }
    if (n_head) c.off(h0, j, 0, 1);
    if (n_rest > 0) {
      c.off(h1, j, n_head, n_rest);
      hipEventRecord(ds.ev_rest, h1.s);
      rest_pending = true;
      if (!head) {   // no look-ahead for this column: diag(j + 1) needs a tile of this launch
        hipStreamWaitEvent(h0.s, ds.ev_rest, 0);
        rest_pending = false;
      }
    }
  }
  if (rest_pending) hipStreamWaitEvent(c.st, ds.ev_rest, 0);
  return check_launch("thx_chol_factor");
}

// RIGHT-LOOKING SCHEDULE for SMALL dense batches (dense L frame without a tile pattern, whole tiles inside the frame, up to
// thx_chol_schedule.right_looking_max_batch problems).  Left-looking, block column j is two dependent launches whose workgroups
// walk K-loops of j tiles -- the diagonal one with ONE workgroup per problem: at 8 ... 64 problems the chip is 3 ... 25 % occupied
// and a factorisation is the sum of those serial K-loops (n = 1536, batch 8: 1.62 ms, 0.04 of the MFMA peak).  Here every tile
// product is its own workgroup: per block column  chol_diag (the tile factorisation alone) -> chol_offdiag as the substitution
// alone, B (ntiles - 1 - j) tiles -> chol_offdiag as the trailing update, B m (m + 1) / 2 tiles each receiving ONE product; the
// working matrix lives in the L frame (first touched by column 0's update, which reads H), the damping of the later diagonal
// tiles is added once after that update.  Same tile kernels, another summation order: the factor differs from the left-looking
// one in the last bits (tests: against LAPACK and against the left-looking solution).  The forward substitution runs as its
// own kernel afterwards.
// (c by value: with the forward substitution fused, y starts as a copy of g and from then on is the kernels' rhs -- c.rhs = y;
// without it the caller runs the forward substitution on the ORIGINAL rhs afterwards, FACTOR_NEEDS_FORWARD)
template <typename T>
static int run_right_looking(FactorLaunch<T> c) {
  DeviceLaunchState& ds = c.ds;
  const hipStream_t st = c.st;
  const int n = c.n, B = c.B, ntiles = c.P.ntiles, hbm = c.P.hbm, dev = c.dev, Bpad = (B + 7) / 8 * 8;
  const int64_t ld = c.ld, ldv = c.ldv;
  const bool use_hb = c.use_hb;
  const HBlk& hb = c.hb;
  const TilePat& pat = c.pat;
    // forward substitution riding on the schedule (vectors with 16-byte rows; else its own kernel afterwards, FACTOR_NEEDS_FORWARD): y starts
    // as a copy of g; chol_diag(j) turns block j into y_j in place, the substitution tiles of column j update the blocks below
  const bool fwd_fused = c.P.rl_fwd_fused;
  if (fwd_fused) {
    hipMemcpy2DAsync(c.y, (size_t)ldv * sizeof(T), c.rhs, (size_t)ldv * sizeof(T), (size_t)n * sizeof(T), (size_t)B, hipMemcpyDeviceToDevice, st);
    c.rhs = c.y;
  }
  TilePat p0 = pat, p1 = pat;
  p1.rl = 1;
  if (fwd_fused) {
    p0.rl_y = p1.rl_y = c.y;
    p0.rl_ldv = p1.rl_ldv = ldv;
  }
  const HBlk nohb{nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0};
  const T* H = (const T*)c.H;
  T *L = (T*)c.L, *panel = (T*)c.panel;
  const T* Lc = L;
  const T* yc = fwd_fused ? (const T*)c.y : nullptr;
  T* yw = fwd_fused ? (T*)c.y : nullptr;
  // (the later columns run the dense-frame instance of chol_diag on the L frame whatever H is)
  const size_t dsm_rl = fwd_fused ? c.dsm : DiagSmem<T>::bytes(0);
  // one chol_offdiag launch: nrt workgroup slots per problem (row tiles / update tiles), H from the block list, the dense H
  // frame or the L frame.  Not FactorLaunch::off: unsplit, the RL instance in fp64, never the half-tile / eight-wave kernels.
  auto off = [&](bool hbsrc, const T* Hsrc, int jarg, int i_first, int nrt, const TilePat& pp, hipStream_t so = nullptr) {
    if (!so) so = st;
    with_hb_mode(hbsrc ? hbm : 0, [&](auto mode) {
      constexpr int M = decltype(mode)::value;
      if constexpr (sizeof(T) == 4)
        launch_lds<chol_offdiag_f32_kernel<M>>(dev, dim3(Bpad * nrt), dim3(256), OFF32_SMEM, so, (const float*)(M ? nullptr : Hsrc),
                                               (float*)L, (const float*)panel, n, ld, jarg, ntiles, i_first, nrt, B, pp, M ? hb : nohb);
      else
        launch_lds<chol_offdiag_f64_kernel<M, true>>(dev, dim3(Bpad * nrt), dim3(256), OFF64_SMEM, so,
                                                     (const double*)(M ? nullptr : Hsrc), (double*)L, (const double*)panel, n, ld, jarg,
                                                     ntiles, i_first, nrt, B, pp, M ? hb : nohb);
    });
  };
  auto upd = [&](int jc, bool first) {
    const int m = ntiles - 1 - jc;
    TilePat pu = pat;
    pu.rl = 2 + jc;
    off(first && use_hb, first ? H : Lc, jc, 0, m * (m + 1) / 2, pu);
  };
  auto damp = [&](int d0) {   // the damping of the diagonal elements d >= d0, once the first trailing update has written them
    if (c.damping && n > d0)
      hipLaunchKernelGGL(rl_damp_kernel<T>, dim3((n - d0 + 255) / 256, B), dim3(256), 0, st, L, ld, H, ld, hb, (const T*)c.damping,
                         c.ellipsoidal, (T)c.eps, d0, n);
  };
  const int la = c.P.rl_mode;
  // block column 0: the kernels as they are (no earlier columns), reading H
  c.diag(Half{st, 0, B}, 0, 1, true, c.dsm);   // (with a right-hand side: y_0 = W_00 g_0 -- kept when the forward substitution is fused)
  off(use_hb, H, 0, 1, ntiles - 1, p0);
  int jstart = 1;
  if (la == 1) {
      // (mode 1) block column 1 the same way, straight from H: chol_diag(1) and the substitution tiles (i, 1) read their tile of H
      // (block list or dense frame; the diagonal tile with its damping) and take column 0's update through the one-tile K-loop;
      // column 0's update of the tiles right of column 1 -- which moves H into the L frame -- rides with the substitutions.
      // (The plain schedule's update(0) is 66 tiles per problem at 12 block columns: 528 workgroups at batch 8, 16 more than one round.)
    TilePat pd1 = p0;
    pd1.rl = 1;
    pd1.rl_la = 1;
    with_bool(use_hb, [&](auto hbk) {
      constexpr bool HB = decltype(hbk)::value;
      launch_lds<chol_diag_kernel<T, HB>>(dev, dim3(B, 1), dim3(256), dsm_rl, st, HB ? (const T*)nullptr : H, L, panel,
                                          (const T*)c.damping, c.ellipsoidal, (T)c.eps, c.info, n, ld, 1, ntiles, yc, yw, ldv, pd1,
                                          HB ? hb : nohb);
    });
    const int nsub = ntiles - 2;
    TilePat pc1 = pd1;
    pc1.rl_nsub = nsub;
    off(use_hb, H, 1, 2, nsub + nsub * (nsub + 1) / 2, pc1);
    damp(2 * TILE);
    jstart = 2;
  } else {
    upd(0, true);
    damp(TILE);
  }
    // MODE 1, TWO LAUNCHES PER BLOCK COLUMN (TilePat.rl_la / rl_nsub; fp32's default; mode 0: the three launches of the plain schedule).
    // The chain per column was diag -> substitutions -> trailing update, although the next diagonal phase and the next
    // substitutions need only ONE block column of that update.  From block column 2 on every tile of column j takes column
    // j - 1's update ITSELF -- chol_diag(j) and the substitution tiles (i, j) run a K-loop over the one tile of column j - 1, the
    // left-looking kernels' own path -- and the rest of that update (tiles (i, k), j < k <= i: needed from column j + 1 on) rides
    // in the SAME chol_offdiag launch as column j's substitutions, as extra workgroup slots:
    //   diag(j) [own update]  ->  { substitutions (i, j) [own update]  +  update of column j - 1 on the tiles right of column j }
    // No second stream, no events.  Another summation order for the tiles' last update (one K-loop product added before the
    // substitution instead of a read-modify-write before it): to rounding, as the schedule itself.
    // MODE 2, the second stream (fp64's default): only chol_diag(j) takes its own update; update(j - 1) is launched without tile
    // (j, j) (first slot skipped) on the library's second stream and runs BESIDE diag(j); the substitutions of column j wait for
    // both.  Hides the whole update instead of the part the substitutions cover, for two event hops per column.
    // MEASURED (profiles/r6/ao_, n = 1536, factor + forward, plain / mode 1 / mode 2): fp32 batch 8 0.742 / 0.724 / 0.756 ms, 16:
    // 0.856 / 0.828 / 0.855, 32: 1.10 / 1.05 / 1.08; fp64 batch 8 1.53 / 1.42 / 1.34, 16: 1.77 / 1.66 / 1.60, 32: 2.41 / 2.28 / 2.19
    // -- an fp32 update launch is as short as the event hops, an fp64 one twice as long.  thx_chol_schedule.right_looking_mode forces
    // a mode.
  hipStream_t sa = st;
  if (la == 2) {
    ds.need_aux();
    sa = ds.aux;
  }
  TilePat pd = p1;
  pd.rl_la = 1;
  bool upd_pending = false;   // (mode 2) an update launch on the second stream that the caller's stream has not waited for yet
  for (int j = jstart; j < ntiles; ++j) {
    launch_lds<chol_diag_kernel<T, false>>(dev, dim3(B, 1), dim3(256), dsm_rl, st, Lc, L, panel, (const T*)nullptr, 0, T(0), c.info, n,
                                           ld, j, ntiles, yc, yw, ldv, (la && j >= 2) ? pd : p1, nohb);
    if (j + 1 == ntiles) break;
    if (la == 0) {
      off(false, Lc, j, j + 1, ntiles - 1 - j, p1);
      upd(j, false);
    } else if (la == 1) {   // (from column 2 on: column 1 ran straight from H above)
      const int nsub = ntiles - 1 - j;
      TilePat pc = pd;
      pc.rl_nsub = nsub;
      off(false, Lc, j, j + 1, nsub + nsub * (nsub + 1) / 2, pc);
    } else {
      if (upd_pending) {   // the substitutions read the tiles update(j - 1) wrote
        hipStreamWaitEvent(st, ds.ev_rest, 0);
        upd_pending = false;
      }
      off(false, Lc, j, j + 1, ntiles - 1 - j, p1);
      const int m = ntiles - 1 - j, nslots = m * (m + 1) / 2 - 1;   // (slot 0 = tile (j + 1, j + 1): left to diag(j + 1))
      if (nslots > 0) {
        hipEventRecord(ds.ev_diag, st);
        hipStreamWaitEvent(sa, ds.ev_diag, 0);
        TilePat pu = pat;
        pu.rl = 2 + j;
        off(false, Lc, j, 1, nslots, pu, sa);
        hipEventRecord(ds.ev_rest, sa);
        upd_pending = true;
      }
    }
  }
  if (upd_pending) hipStreamWaitEvent(st, ds.ev_rest, 0);
  if (int r = check_launch("thx_chol_factor (right-looking)")) return r;
  return (c.rhs && !fwd_fused) ? FACTOR_NEEDS_FORWARD : 0;   // (the caller runs the forward substitution as its own kernel)
}

// LEFT-LOOKING, column by column: plain, in column pairs (P.colpair, see plan_factor) and, from SPLIT_MIN problems on, two streams:
// One half of the batch per stream, the second half one diagonal phase behind the first: the latency-bound serial part
// of chol_diag (one wave per workgroup busy, §4.1) and the tail of every launch of one half run underneath the MFMA-bound
// chol_offdiag of the other half.  The halves touch disjoint memory; the auxiliary stream forks from / joins the
// caller's stream through events.  (Overlapping diag(j+1) with the rest of column j of the SAME problems had gained
// nothing: column j+1 needs all of column j, so there is no slack to fill.)
template <typename T>
static int run_left_looking(const FactorLaunch<T>& c) {
  const thx_tile_pattern* tp = c.tp;
  DeviceLaunchState& ds = c.ds;
  const int B = c.B, ntiles = c.P.ntiles;
  const bool split = c.P.split;
  Half halves[2] = {{c.st, 0, B}, {c.st, 0, 0}};
  if (split) {
    ds.need_aux();
    const int per = min((B / 2 + 7) / 8 * 8, B);  // (multiple of 8: the XCD-aware block map of chol_offdiag)
    halves[0] = {c.st, 0, per};
    halves[1] = {ds.aux, per, B - per};
    hipEventRecord(ds.ev_fork, c.st);
    hipStreamWaitEvent(ds.aux, ds.ev_fork, 0);
  }
  for (int j = 0; j < ntiles;) {
    const bool pair = c.P.colpair && j + 2 < ntiles;
    for (int k = 0; k < c.P.nparts; ++k) {
      const Half& h = halves[k];
      if (h.nb <= 0) continue;
      if (split && k == 1 && j == 0) hipStreamWaitEvent(h.s, ds.ev_lag, 0);  // half 1: one diagonal phase behind half 0
      c.diag(h, j);
      if (split && k == 0 && j == 0) hipEventRecord(ds.ev_lag, h.s);
      if (pair) {
        c.head(h, j);
        c.diag(h, j + 1);
        const int32_t* gp = c.P.regroup ? c.hb.rg_group_ptr_host : nullptr;
        const int g0 = gp ? gp[j / 2] : 0, ng = gp ? gp[j / 2 + 1] - g0 : 0;
        if (ng > 0) c.pair_groups(h, j, g0, ng);
        else if (j == 0 && c.P.pair0) c.pair_groups0(h);
        else c.pair(h, j, j + 2, ntiles - 2 - j);
        continue;
      }
      const int nrt = tp ? tp->col_count_host[j] : ntiles - 1 - j;   // (tile-sparse: the column's non-zero row tiles)
      // (an even last-but-one column of the pair schedule is a head tile without a pair behind it)
      if (nrt == 1 && !tp && c.P.colpair && j % 2 == 0) c.head(h, j);
      else if (nrt > 0) c.off(h, j, tp ? 0 : j + 1, nrt);
    }
    j += pair ? 2 : 1;
  }
  if (split) {
    hipEventRecord(ds.ev_join, ds.aux);
    hipStreamWaitEvent(c.st, ds.ev_join, 0);
  }
  return check_launch("thx_chol_factor");
}

// Checks what the kernels cannot, plans, and enqueues the plan's schedule -- holding g_launch_mutex for the whole enqueue (the
// auxiliary stream / events and the LDS limits are shared).  Nothing below may call solve_impl, which takes the lock itself.
template <typename T>
static int factor_impl(const void* H, int64_t ld, int n, int B, const void* damping, int ellipsoidal, double eps,
                       void* L, void* panel, int32_t* info, const void* rhs, void* y, int64_t ldv, hipStream_t st,
                       const thx_tile_pattern* tp = nullptr, const HBlk* hbp = nullptr, const thx_level_schedule* ls = nullptr,
                       const thx_chol_schedule* sched = nullptr) {
  const bool use_hb = hbp != nullptr;
  const bool packed = ld == 0;   // L is the TILE-PACKED factor (B, nslots, TILE, TILE) of the pattern
  const FactorPlan P = plan_factor(sizeof(T) == 8, n, ld, B, damping != nullptr, rhs != nullptr, ldv,
                                   (reinterpret_cast<uintptr_t>(y) % 16) == 0, tp, hbp, ls, sched);
  const int ntiles = P.ntiles;
  if (packed && (!tp || tp->nslots <= 0 || !tp->tile_sa || !tp->tile_sb || !tp->diag_s))
    return fail("thx_chol_factor: a tile-packed factor (ld = 0) needs a tile pattern with slot tables");
  if (tp && tp->ntiles != ntiles) return fail("thx_chol_factor_sparse: the tile pattern was built for another matrix order");
  const int64_t lstride = packed ? (int64_t)tp->nslots * TILE * TILE : (int64_t)ld * ld;
  if (packed && lstride * (int64_t)sizeof(T) > 0x7fffffffLL)
    return fail("thx_chol_factor: tile-packed factor larger than 2 GB per problem");
  const size_t dsm = P.fused_diag ? DiagSmem<T>::bytes(rhs ? ntiles * TILE : 0) : SyrkSmem<T>::bytes(rhs ? ntiles * TILE : 0);
  if (dsm > LDS_LIMIT) return fail("thx_chol_factor: n too large for the fused forward substitution (LDS)");
  if (ls && (!packed || !use_hb)) return fail("thx_chol_factor_levels: tile-packed factor + block-compact H");
  if (ls && rhs)   // (run_levels sizes the launch of level l for the longest K-list of that level)
    for (int l = 0; l < ls->nlevels; ++l) {
      const int yp = ls->level_maxk_host[l] * TILE;
      if (std::max(DiagSmem<T>::bytes(yp), SyrkSmem<T>::bytes(yp)) > LDS_LIMIT)
        return fail("thx_chol_factor_levels: K-list too long for the fused forward substitution (LDS)");
    }
  // (lpt: the level's / column's entries are sorted longest K-list first; consecutive workgroups = the problems of one entry)
  const int lpt = (P.schedule == Schedule::Levels || P.schedule == Schedule::LookAhead) ? 1 : 0;
  TilePat pat{};
  if (tp)
    pat = TilePat{tp->col_ptr, tp->col_row, tp->tile_kptr, tp->tile_k, tp->diag_kptr, tp->diag_k,
                  packed ? tp->tile_sa : nullptr, packed ? tp->tile_sb : nullptr, packed ? tp->diag_s : nullptr,
                  packed ? tp->nslots : 0, lpt, ls ? ls->ent_col : nullptr, ls ? ls->tile_valid : nullptr};
  HBlk hb = use_hb ? *hbp : HBlk{};
  if (!P.zskip) hb.l_mask = nullptr;
  if (!P.regroup) hb.rg_rows = hb.rg_k0 = hb.rg_tile_ptr = hb.rg_piece_blk = hb.rg_piece_rc = nullptr;
  if (!P.zsolve || !P.regroup) hb.rg_zf = nullptr;
  if (!P.sortcols) hb.sc_perm = hb.sc_mask = hb.sc_pair_host = nullptr;
  if (!P.sortrows) hb.tr_perm16 = hb.tr_mask16 = hb.tr_tile_host = nullptr;
  if (!P.sorthead) hb.th_perm32 = hb.th_mask32 = hb.th_k0h = hb.th_tile_host = nullptr;
  std::lock_guard<std::mutex> guard(g_launch_mutex);
  const int dev = current_device();
  const FactorLaunch<T> c{H, ld, n, B, damping, ellipsoidal, eps, L, panel, info, rhs, y, ldv, st, tp, ls, P, pat, use_hb, hb, packed,
                          (int64_t)ld * ld, lstride, dsm, dev, launch_state(dev)};
  hipMemsetAsync(info, 0, sizeof(int32_t) * (size_t)B, st);
  switch (P.schedule) {
    case Schedule::Levels: return run_levels(c);
    case Schedule::LookAhead: return run_lookahead(c);
    case Schedule::RightLooking: return run_right_looking(c);
    default: return run_left_looking(c);
  }
}

template <typename T>
static int solve_impl(const void* L, int64_t ld, int n, int B, const void* panel, const void* rhs, void* x,
                      int64_t ldv, bool forward, bool backward, hipStream_t st, const thx_tile_pattern* tp = nullptr,
                      const thx_level_schedule* ls = nullptr, const int32_t* row_first = nullptr) {
  const int ntiles = (n + TILE - 1) / TILE;
  const bool list = tp != nullptr;
  const bool env = row_first != nullptr && !list;   // the envelope path of the dense-frame kernels (thx_chol_solve_env)
  const size_t sm = solve_smem<T>(list ? 0 : ntiles * TILE, env);
  if (sm > LDS_LIMIT) return fail("thx_chol_solve: n too large for the LDS plan (thx_chol_solve_sparse has no limit)");
  const bool packed = ld == 0;
  if (packed && (!list || !tp->row_slot || tp->nslots <= 0))
    return fail("thx_chol_solve: a tile-packed factor (ld = 0) needs thx_chol_solve_sparse and a pattern with slot tables");
  if (ls && !list) return fail("thx_chol_solve_levels: needs the tile pattern");
  RowPat rp{list ? tp->row_ptr : nullptr, list ? tp->row_tile : nullptr, packed ? tp->row_slot : nullptr, packed ? tp->nslots : 0,
            -1, ls ? ls->tile_valid : nullptr};
  std::lock_guard<std::mutex> guard(g_launch_mutex);   // (the LDS limits; not recursive -- see factor_then_forward)
  const int dev = current_device();
  const T* src = (const T*)rhs;
  auto copy_to_x = [&] {   // the backward substitution runs in place
    if (src != (const T*)x)
      hipMemcpy2DAsync(x, (size_t)ldv * sizeof(T), src, (size_t)ldv * sizeof(T), (size_t)n * sizeof(T), (size_t)B,
                       hipMemcpyDeviceToDevice, st);
  };
  if (ls) {
    // LEVEL SCHEDULE: one launch per elimination-tree level, one workgroup per (problem, block row of the level) -- forward bottom
    // up (a row pulls from its descendants' blocks of y), backward top down (a row pushes into its descendants' blocks of x)
    if (forward) {
      for (int l = 0; l < ls->nlevels; ++l) {
        rp.j0 = ls->level_col_host[l];
        const int nc = ls->level_col_host[l + 1] - rp.j0;
        if (nc > 0)
          launch_lds<chol_fwd_kernel<T, true>>(dev, dim3(B, nc), dim3(256), sm, st, (const T*)L, (const T*)panel, src, (T*)x, n, ld, ldv,
                                               ntiles, rp, nullptr);
      }
      src = (const T*)x;
    }
    if (backward) {
      copy_to_x();
      for (int l = ls->nlevels - 1; l >= 0; --l) {
        rp.j0 = ls->level_col_host[l];
        const int nc = ls->level_col_host[l + 1] - rp.j0;
        if (nc > 0)
          launch_lds<chol_bwd_kernel<T, true>>(dev, dim3(B, nc), dim3(256), sm, st, (const T*)L, (const T*)panel, (const T*)x, (T*)x, n,
                                               ld, ldv, ntiles, rp, nullptr);
      }
    }
    return check_launch("thx_chol_solve_levels");
  }
  if (forward) {
    if (env)
      launch_lds<chol_fwd_kernel<T, false, true>>(dev, dim3(B), dim3(256), sm, st, (const T*)L, (const T*)panel, src, (T*)x, n, ld, ldv,
                                                  ntiles, rp, row_first);
    else
      with_bool(list, [&](auto lk) {
        launch_lds<chol_fwd_kernel<T, decltype(lk)::value>>(dev, dim3(B), dim3(256), sm, st, (const T*)L, (const T*)panel, src, (T*)x, n,
                                                            ld, ldv, ntiles, rp, nullptr);
      });
    src = (const T*)x;  // the backward pass then runs in place
  }
  // small batches, dense frame: one launch per block row (chol_bwd_rows_kernel; bit-identical to chol_bwd_kernel) -- up to
  // BWD_ROWS_MAX_BATCH problems per call.  A SMALL gain: chol_bwd_kernel's push already runs 256 threads
  // x 8 loads deep (n = 1536, batch 8: 115 us; block rows: 101 us, twelve launches of 5.5 ... 9 us; no difference from 64
  // problems on, profiles/r6/o_ab_bwd_rows.txt) -- it is chol_fwd_kernel's row dots that take 0.46 ms at any batch size, and
  // the right-looking schedule fuses the forward substitution instead.
  if (backward && !list && ntiles >= 3 && B <= BWD_ROWS_MAX_BATCH) {
    copy_to_x();
    const size_t smr = solve_smem<T>(0);
    for (int jb = ntiles; jb >= 1; --jb)
      launch_lds<chol_bwd_rows_kernel<T>>(dev, dim3(jb < ntiles ? jb : 1, B), dim3(256), smr, st, (const T*)L, (const T*)panel, (T*)x, n,
                                          ld, ldv, ntiles, jb);
    return check_launch("thx_chol_solve (block rows)");
  }
  if (backward && env)
    launch_lds<chol_bwd_kernel<T, false, true>>(dev, dim3(B), dim3(256), sm, st, (const T*)L, (const T*)panel, src, (T*)x, n, ld, ldv,
                                                ntiles, rp, row_first);
  else if (backward)
    with_bool(list, [&](auto lk) {
      launch_lds<chol_bwd_kernel<T, decltype(lk)::value>>(dev, dim3(B), dim3(256), sm, st, (const T*)L, (const T*)panel, src, (T*)x, n,
                                                          ld, ldv, ntiles, rp, nullptr);
    });
  return check_launch("thx_chol_solve");
}

// factor_impl + (right-looking schedule: return code FACTOR_NEEDS_FORWARD) the forward substitution as its own kernel -- outside factor_impl's
// launch lock, which solve_impl takes itself
template <typename T, typename... A>
static int factor_then_forward(const void* H, int64_t ld, int n, int B, const void* damping, int ellipsoidal, double eps, void* L,
                               void* panel, int32_t* info, const void* rhs, void* y, int64_t ldv, hipStream_t st, A... more) {
  const int r = factor_impl<T>(H, ld, n, B, damping, ellipsoidal, eps, L, panel, info, rhs, y, ldv, st, more...);
  if (r != FACTOR_NEEDS_FORWARD) return r;
  return solve_impl<T>(L, ld, n, B, panel, rhs, y, ldv, true, false, st);
}

}  // namespace thx

using namespace thx;

extern "C" {

static int check_factor_args(const void* H, const void* L, const void* panel, const void* info, int n, int B,
                             int64_t ld) {
  if (!H || !L || !panel || !info) return fail("thx_chol_factor: null pointer");
  if (n <= 0 || B <= 0 || (ld != 0 && (ld < n || (ld % 32) != 0)))
    return fail("thx_chol_factor: need n>0, B>0, ld>=n, ld%32==0 (ld = 0: tile-packed factor)");
  return 0;
}

// the tile-pattern tables every tile-sparse factorisation reads
static int check_pattern(const thx_tile_pattern* pattern, const char* who) {
  if (!pattern || !pattern->col_ptr || !pattern->col_row || !pattern->tile_kptr || !pattern->tile_k || !pattern->diag_kptr ||
      !pattern->diag_k || !pattern->col_count_host)
    return fail(who, ": incomplete tile pattern");
  return 0;
}

// the right-hand side and its forward-substituted vector: both or (unless `required`) neither, of at least n elements, not aliased
static int check_rhs(const void* rhs, const void* y, int64_t ldv, int n, const char* who, bool required = false,
                     const char* what = ": rhs / y / ldv") {
  if (required ? (!rhs || !y || ldv < n) : ((rhs == nullptr) != (y == nullptr) || (rhs && ldv < n))) return fail(who, what);
  if (rhs && rhs == y) return fail(who, ": y must not alias rhs");
  return 0;
}

// the kernels' view of a block-compact Hessian: the layout's tables and the value buffer (B, bstride)
static HBlk hblk_from(const thx_hblock_layout* layout, const void* Hc, int64_t bstride) {
  return HBlk{Hc, bstride, layout->bd, layout->tile_ptr, layout->piece_blk, layout->piece_rc, layout->diag_blk, layout->max_tile_pieces,
              layout->l_mask, layout->rg_rows, layout->rg_k0, layout->rg_tile_ptr, layout->rg_piece_blk, layout->rg_piece_rc,
              layout->rg_group_ptr_host, layout->rg_max_tile_pieces, layout->rg_zf, layout->rg0_rows, layout->rg0_zf, layout->rg0_tile_ptr,
              layout->rg0_piece_blk, layout->rg0_piece_rc, layout->rg0_ngroups, layout->rg0_max_tile_pieces, layout->sc_perm,
              layout->sc_mask, layout->sc_pair_host, layout->tr_perm16, layout->tr_mask16, layout->tr_tile_host,
              layout->th_perm32, layout->th_mask32, layout->th_k0h, layout->th_tile_host};
}

int thx_chol_factor(const void* H, int64_t ld, int32_t n, int32_t B, const void* damping, int ellipsoidal,
                    double damping_eps, void* L, void* Winv, int32_t* info, int dtype, void* stream, const thx_chol_schedule* schedule) {
  if (int r = check_factor_args(H, L, Winv, info, n, B, ld)) return r;
  THX_DISPATCH(dtype,
               return factor_then_forward<float>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, nullptr,
                                         nullptr, 0, as_stream(stream), nullptr, nullptr, nullptr, schedule),
               return factor_then_forward<double>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, nullptr,
                                          nullptr, 0, as_stream(stream), nullptr, nullptr, nullptr, schedule));
  return 0;
}

int thx_chol_factor_forward(const void* H, int64_t ld, int32_t n, int32_t B, const void* damping, int ellipsoidal,
                            double damping_eps, void* L, void* Winv, int32_t* info, const void* rhs, void* y,
                            int64_t ldv, int dtype, void* stream, const thx_chol_schedule* schedule) {
  if (int r = check_factor_args(H, L, Winv, info, n, B, ld)) return r;
  if (int r = check_rhs(rhs, y, ldv, n, "thx_chol_factor_forward", true)) return r;
  THX_DISPATCH(dtype,
               return factor_then_forward<float>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                         as_stream(stream), nullptr, nullptr, nullptr, schedule),
               return factor_then_forward<double>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                          as_stream(stream), nullptr, nullptr, nullptr, schedule));
  return 0;
}

int thx_chol_factor_sparse(const void* H, int64_t ld, int32_t n, int32_t B, const void* damping, int ellipsoidal,
                           double damping_eps, void* L, void* Winv, int32_t* info, const void* rhs, void* y, int64_t ldv,
                           const thx_tile_pattern* pattern, int dtype, void* stream, const thx_chol_schedule* schedule) {
  if (int r = check_factor_args(H, L, Winv, info, n, B, ld)) return r;
  if (ld == 0) return fail("thx_chol_factor_sparse: H is a dense frame here (ld >= n); the tile-packed factor goes with thx_chol_factor_hblocks");
  if (int r = check_pattern(pattern, "thx_chol_factor_sparse")) return r;
  if (int r = check_rhs(rhs, y, ldv, n, "thx_chol_factor_sparse")) return r;
  THX_DISPATCH(dtype,
               return factor_impl<float>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                         as_stream(stream), pattern, nullptr, nullptr, schedule),
               return factor_impl<double>(H, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                          as_stream(stream), pattern, nullptr, nullptr, schedule));
  return 0;
}

static int solve_dispatch(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x,
                          int64_t ldv, bool fwd, bool bwd, int dtype, void* stream, const thx_tile_pattern* tp = nullptr,
                          const int32_t* row_first = nullptr) {
  if (!L || !Winv || !rhs || !x) return fail("thx_chol_solve: null pointer");
  if (n <= 0 || B <= 0 || (ld != 0 && ld < n) || ldv < n) return fail("thx_chol_solve: bad sizes");
  THX_DISPATCH(dtype, return solve_impl<float>(L, ld, n, B, Winv, rhs, x, ldv, fwd, bwd, as_stream(stream), tp, nullptr, row_first),
               return solve_impl<double>(L, ld, n, B, Winv, rhs, x, ldv, fwd, bwd, as_stream(stream), tp, nullptr, row_first));
  return 0;
}

int thx_chol_solve_sparse(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x,
                          int64_t ldv, int backward_only, const thx_tile_pattern* pattern, int dtype, void* stream) {
  if (!pattern || !pattern->row_ptr || !pattern->row_tile) return fail("thx_chol_solve_sparse: incomplete tile pattern");
  if (pattern->ntiles != (n + TILE - 1) / TILE) return fail("thx_chol_solve_sparse: the pattern is not this matrix's");
  return solve_dispatch(L, ld, n, B, Winv, rhs, x, ldv, !backward_only, true, dtype, stream, pattern);
}

int thx_chol_factor_hblocks(const thx_hblock_layout* layout, const void* Hc, int64_t bstride, int32_t n, int32_t B,
                            const void* damping, int ellipsoidal, double damping_eps, void* L, int64_t ld, void* Winv,
                            int32_t* info, const void* rhs, void* y, int64_t ldv, const thx_tile_pattern* pattern, int dtype,
                            void* stream, const thx_chol_schedule* schedule) {
  if (!layout || !layout->tile_ptr || !layout->piece_blk || !layout->piece_rc || !Hc)
    return fail("thx_chol_factor_hblocks: incomplete block layout");
  if (int r = check_factor_args(Hc, L, Winv, info, n, B, ld)) return r;
  if (layout->ntiles != (n + TILE - 1) / TILE || layout->nvars * layout->bd != n || bstride < (int64_t)layout->nblocks * layout->bd * layout->bd)
    return fail("thx_chol_factor_hblocks: the block layout is not this matrix's");
  if (pattern)
    if (int r = check_pattern(pattern, "thx_chol_factor_hblocks")) return r;
  if (int r = check_rhs(rhs, y, ldv, n, "thx_chol_factor_hblocks")) return r;
  const HBlk hb = hblk_from(layout, Hc, bstride);
  THX_DISPATCH(dtype,
               return factor_then_forward<float>(nullptr, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                         as_stream(stream), pattern, &hb, nullptr, schedule),
               return factor_then_forward<double>(nullptr, ld, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                          as_stream(stream), pattern, &hb, nullptr, schedule));
  return 0;
}

int thx_chol_plan(int32_t n, int64_t ld, int32_t B, int dtype, int has_damping, int has_rhs, int64_t ldv,
                  const thx_hblock_layout* layout, const thx_chol_schedule* schedule, thx_chol_plan_info* out) {
  if (!out) return fail("thx_chol_plan: null pointer");
  if (n <= 0 || B <= 0 || ld < n || (ld % 32) != 0) return fail("thx_chol_plan: need n>0, B>0, ld>=n, ld%32==0 (dense factor frame)");
  if (has_rhs && ldv < n) return fail("thx_chol_plan: ldv < n");
  if (dtype != THX_F32 && dtype != THX_F64) return fail("bad dtype");
  if (layout && layout->ntiles != (n + TILE - 1) / TILE) return fail("thx_chol_plan: the block layout is not this matrix's");
  HBlk hb = layout ? hblk_from(layout, nullptr, 0) : HBlk{};   // (no data pointers: the plan reads bd, the piece maxima, which tables are set)
  const FactorPlan p = plan_factor(dtype == THX_F64, n, ld, B, has_damping != 0, has_rhs != 0, ldv, true, nullptr,
                                   layout ? &hb : nullptr, nullptr, schedule);
  const bool rl = p.schedule == Schedule::RightLooking;
  out->right_looking = rl;
  out->right_looking_mode = rl ? p.rl_mode : -1;
  out->split_diag = !p.fused_diag;
  out->nparts = p.nparts;
  out->column_pairs = p.colpair;
  // (fp64 off-diagonal launches of the column-by-column schedule: block columns 0 .. ntiles - 2; the half-tile kernel first, then the
  //  eight-wave one -- FactorLaunch::off; neither takes the LDS gather rounds of a block list)
  const int cols = p.ntiles - 1;
  const bool f64_lanes = dtype == THX_F64 && !rl && p.hbm != HB_MODE_ROUNDS;
  const int half = f64_lanes ? std::max(0, std::min(p.f64_half_max, cols)) : 0;
  out->f64_half_cols = half;
  out->f64_wide_cols = f64_lanes ? std::max(0, std::min(p.f64_wide_max, cols) - half) : 0;
  out->forward_fused = has_rhs && (!rl || p.rl_fwd_fused);
  out->regroup_rows = p.regroup;
  out->skip_zero_solves = p.zsolve;
  out->sort_pair_columns = p.sortcols;
  out->sort_tile_rows = p.sortrows || p.sorthead;
  return 0;
}

// Natural-order symbolic Cholesky of the variable-block pattern (Liu's row-subtree walk: row p of L is the union of the elimination-tree
// paths from the columns q < p of row p of H up to p; the tree grows as the rows are visited), reduced to the l_mask table.
int thx_hblock_fill_mask(int32_t nvars, int32_t bd, int32_t nblocks, const int32_t* blocks, int32_t* mask) {
  if (nvars <= 0 || bd <= 0 || nblocks < 0 || (nblocks > 0 && !blocks) || !mask) return fail("thx_hblock_fill_mask: bad arguments");
  const int64_t n = (int64_t)nvars * bd;
  if (n > (int64_t)1 << 24) return fail("thx_hblock_fill_mask: matrix too large");
  const int ntiles = (int)((n + TILE - 1) / TILE), nch = 4 * ntiles;
  std::vector<int32_t> rptr(nvars + 1, 0), rcol;
  for (int32_t e = 0; e < nblocks; ++e) {
    const int32_t p = blocks[2 * e], q = blocks[2 * e + 1];
    if (p < 0 || p >= nvars || q < 0 || q > p) return fail("thx_hblock_fill_mask: a block outside tril(H)");
    if (q < p) ++rptr[p + 1];
  }
  for (int32_t v = 0; v < nvars; ++v) rptr[v + 1] += rptr[v];
  rcol.resize(rptr[nvars]);
  {
    std::vector<int32_t> fill(rptr.begin(), rptr.end() - 1);
    for (int32_t e = 0; e < nblocks; ++e)
      if (blocks[2 * e + 1] < blocks[2 * e]) rcol[fill[blocks[2 * e]]++] = blocks[2 * e + 1];
  }
  std::fill(mask, mask + (int64_t)ntiles * nch, 0);
  // block (p, q) of L, q <= p: every 32 x 32 sub-block (R, C), R >= C, that its rows / columns overlap
  auto mark = [&](int32_t p, int32_t q) {
    const int64_t r0 = (int64_t)p * bd, c0 = (int64_t)q * bd;
    for (int64_t R = r0 / 32; R <= (r0 + bd - 1) / 32; ++R)
      for (int64_t C = c0 / 32; C <= std::min((c0 + bd - 1) / 32, R); ++C) mask[(R / 4) * nch + C] |= 1 << (R % 4);
  };
  std::vector<int32_t> parent(nvars, -1), flag(nvars, -1);
  for (int32_t p = 0; p < nvars; ++p) {
    flag[p] = p;
    mark(p, p);
    for (int32_t e = rptr[p]; e < rptr[p + 1]; ++e)
      for (int32_t k = rcol[e]; flag[k] != p; k = parent[k]) {
        if (parent[k] < 0) parent[k] = p;
        flag[k] = p;
        mark(p, k);
      }
  }
  return 0;
}

static int check_levels(const thx_tile_pattern* pattern, const thx_level_schedule* ls, const char* who) {
  if (!pattern || !pattern->col_ptr || !pattern->col_row || !pattern->tile_kptr || !pattern->tile_k || !pattern->diag_kptr ||
      !pattern->diag_k || !pattern->row_ptr || !pattern->row_tile || !pattern->tile_sa || !pattern->tile_sb || !pattern->diag_s ||
      !pattern->row_slot || pattern->nslots <= 0 || pattern->ntiles <= 0)
    return fail(who, ": incomplete tile pattern (the level schedule works on the tile-packed factor)");
  if (!ls || ls->nlevels <= 0 || !ls->level_col_host || !ls->level_ent_host || !ls->level_maxk_host || !ls->ent_col || !ls->tile_valid)
    return fail(who, ": incomplete level schedule");
  if (ls->level_col_host[0] != 0 || ls->level_col_host[ls->nlevels] != pattern->ntiles || ls->level_ent_host[0] != 0 ||
      ls->level_ent_host[ls->nlevels] != pattern->nslots - pattern->ntiles)
    return fail(who, ": the level schedule does not cover the pattern's block columns / entries");
  for (int l = 0; l < ls->nlevels; ++l)
    if (ls->level_col_host[l + 1] < ls->level_col_host[l] || ls->level_ent_host[l + 1] < ls->level_ent_host[l] ||
        ls->level_col_host[l + 1] - ls->level_col_host[l] > 65535)
      return fail(who, ": level tables must be non-decreasing, at most 65535 block columns per level");
  return 0;
}

int thx_chol_factor_levels(const thx_hblock_layout* layout, const void* Hc, int64_t bstride, int32_t B, const void* damping,
                           int ellipsoidal, double damping_eps, void* L, void* Winv, int32_t* info, const void* rhs, void* y,
                           int64_t ldv, const thx_tile_pattern* pattern, const thx_level_schedule* schedule, int dtype,
                           void* stream, const thx_chol_schedule* chol_schedule) {
  if (!layout || !layout->tile_ptr || !layout->piece_blk || !layout->piece_rc || !Hc || !L || !Winv || !info || B <= 0)
    return fail("thx_chol_factor_levels: null pointer / incomplete block layout / B <= 0");
  if (int r = check_levels(pattern, schedule, "thx_chol_factor_levels")) return r;
  if (layout->ntiles != pattern->ntiles || bstride < (int64_t)layout->nblocks * layout->bd * layout->bd)
    return fail("thx_chol_factor_levels: the block layout is not this pattern's");
  const int n = pattern->ntiles * TILE;   // (the padded order: every tile is whole, tile_valid says how much of it is matrix)
  if (int r = check_rhs(rhs, y, ldv, n, "thx_chol_factor_levels", false, ": rhs / y are vectors of the PADDED order (ldv >= ntiles * THX_TILE)"))
    return r;
  HBlk hb = hblk_from(layout, Hc, bstride);
  hb.diag_blk = hb.l_mask = nullptr;   // (the level schedule has no right-looking damping pass and skips no sub-blocks)
  THX_DISPATCH(dtype,
               return factor_impl<float>(nullptr, 0, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                         as_stream(stream), pattern, &hb, schedule, chol_schedule),
               return factor_impl<double>(nullptr, 0, n, B, damping, ellipsoidal, damping_eps, L, Winv, info, rhs, y, ldv,
                                          as_stream(stream), pattern, &hb, schedule, chol_schedule));
  return 0;
}

int thx_chol_solve_levels(const void* L, int32_t B, const void* Winv, const void* rhs, void* x, int64_t ldv, int which,
                          const thx_tile_pattern* pattern, const thx_level_schedule* schedule, int dtype, void* stream) {
  if (!L || !Winv || !rhs || !x || B <= 0 || B > 65535) return fail("thx_chol_solve_levels: null pointer / B out of range");
  if (which < 0 || which > 2) return fail("thx_chol_solve_levels: which = 0 (both), 1 (backward only), 2 (forward only)");
  if (int r = check_levels(pattern, schedule, "thx_chol_solve_levels")) return r;
  const int n = pattern->ntiles * TILE;
  if (ldv < n) return fail("thx_chol_solve_levels: rhs / x are vectors of the PADDED order, ldv >= ntiles * THX_TILE");
  THX_DISPATCH(dtype,
               return solve_impl<float>(L, 0, n, B, Winv, rhs, x, ldv, which != 1, which != 2, as_stream(stream), pattern, schedule),
               return solve_impl<double>(L, 0, n, B, Winv, rhs, x, ldv, which != 1, which != 2, as_stream(stream), pattern, schedule));
  return 0;
}

int thx_vec_gather(const void* src, int64_t lds, void* dst, int64_t ldd, const int32_t* idx, int32_t n, int32_t B, int dtype,
                   void* stream) {
  if (!src || !dst || !idx || n <= 0 || B <= 0 || B > 65535 || src == dst) return fail("thx_vec_gather: bad args");
  dim3 grid((n + 255) / 256, B), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(vec_gather_kernel<float>, grid, block, 0, as_stream(stream), (const float*)src, lds, (float*)dst,
                                  ldd, idx, n),
               hipLaunchKernelGGL(vec_gather_kernel<double>, grid, block, 0, as_stream(stream), (const double*)src, lds,
                                  (double*)dst, ldd, idx, n));
  return check_launch("thx_vec_gather");
}

int thx_chol_solve_env(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x,
                       int64_t ldv, const int32_t* row_first, int dtype, void* stream) {
  return solve_dispatch(L, ld, n, B, Winv, rhs, x, ldv, true, true, dtype, stream, nullptr, row_first);
}

int thx_chol_solve_backward_env(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* y, void* x,
                                int64_t ldv, const int32_t* row_first, int dtype, void* stream) {
  return solve_dispatch(L, ld, n, B, Winv, y, x, ldv, false, true, dtype, stream, nullptr, row_first);
}

int thx_chol_solve(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* rhs, void* x,
                   int64_t ldv, int dtype, void* stream) {
  return thx_chol_solve_env(L, ld, n, B, Winv, rhs, x, ldv, nullptr, dtype, stream);
}

int thx_chol_solve_backward(const void* L, int64_t ld, int32_t n, int32_t B, const void* Winv, const void* y, void* x,
                            int64_t ldv, int dtype, void* stream) {
  return thx_chol_solve_backward_env(L, ld, n, B, Winv, y, x, ldv, nullptr, dtype, stream);
}

int thx_diag(const void* H, int64_t ld, int32_t n, int32_t B, void* d, int64_t ldv, int dtype, void* stream) {
  if (!H || !d || n <= 0 || B <= 0) return fail("thx_diag: bad args");
  dim3 grid((n + 255) / 256, B), block(256);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(diag_kernel<float>, grid, block, 0, as_stream(stream), (const float*)H, ld, n,
                                  (float*)d, ldv),
               hipLaunchKernelGGL(diag_kernel<double>, grid, block, 0, as_stream(stream), (const double*)H, ld, n,
                                  (double*)d, ldv));
  return check_launch("thx_diag");
}

int thx_lm_accept(const void* delta, const void* g, int64_t ldv, const void* H, int64_t ld, int32_t n, int32_t B,
                  void* damping, const void* prev_err, const void* new_err, int ellipsoidal, double accept,
                  double down_ratio, double up_ratio, uint8_t* reject, int dtype, void* stream) {
  if (!delta || !g || !damping || !prev_err || !new_err || !reject || (ellipsoidal && !H))
    return fail("thx_lm_accept: null pointer");
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(lm_accept_kernel<float>, dim3(B), dim3(64), 0, as_stream(stream), (const float*)delta,
                                  (const float*)g, ldv, (const float*)H, ld, n, (float*)damping,
                                  (const float*)prev_err, (const float*)new_err, ellipsoidal, (float)accept,
                                  (float)down_ratio, (float)up_ratio, reject),
               hipLaunchKernelGGL(lm_accept_kernel<double>, dim3(B), dim3(64), 0, as_stream(stream),
                                  (const double*)delta, (const double*)g, ldv, (const double*)H, ld, n,
                                  (double*)damping, (const double*)prev_err, (const double*)new_err, ellipsoidal,
                                  accept, down_ratio, up_ratio, reject));
  return check_launch("thx_lm_accept");
}

}  // extern "C"
