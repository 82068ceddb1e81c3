// Batched BANDED Cholesky for chain-structured objectives (trajectories, odometry chains), gfx950: P (H + damping) P^T = L L^T
// with half-bandwidth kd <= BAND_MAX_KD = 63 -- n kd^2 / 2 flops per problem instead of the dense factor's n^3 / 3, one launch.
// The counterpart of LAPACK's pbtrf / pbtrs on the dense (B, ld, ld) frame the assembly kernels write.
//
// ONE WAVE PER PROBLEM (up to four problems per workgroup; the waves never synchronise with each other).
//   band_factor_kernel   column by column.  The live part of the matrix is the (kd + 1) x (kd + 1) trailing window.  What sits in
//                        LDS for it is not the partly updated matrix but the SUMS of products still to be subtracted, a ring of
//                        kd + 1 columns (slot c mod (kd + 1) holds elements (c .. c + kd, c), stride S = (kd + 1) | 1 elements):
//                        an element is a - sum, formed once when its column is reached, so its error is one rounding of a plus
//                        the error of a dot product -- the figure of a blocked potrf -- where subtracting update by update rounds
//                        against the size of a every time (at kd = 63, fp64, that gave 6 x LAPACK's factor residual: DESIGN.md 4.17).  The band of H
//                        is gathered through perm eight columns at a time into registers, ONE CHUNK AHEAD of the chunk being
//                        factorised (the two dependent loads, perm then H, fly under eight column steps), and parked in a second
//                        ring of 16 columns; damping goes onto the diagonal on the way in.
//                        Per column j: every lane forms the pivot (two LDS broadcasts), the lane that owns row j + i forms and
//                        scales element i -- row r belongs to lane r mod 64, so a row keeps its lane for its whole life and the
//                        fused forward substitution below needs no shifts -- writes it to LDS and to Lb[j, 0..kd], one contiguous
//                        segment, and clears its sum (the slot is column j + kd + 1's next); then the rank-1 update of the sums of
//                        the window's lower triangle, kd (kd + 1) / 2 elements folded into a ceil(kd / 2) x (kd + 1) rectangle
//                        (row p with row kd + 1 - p) that is dealt over all 64 lanes: an element's (row, column) follows from a
//                        division done once per kernel and an increment per step.
//                        With rhs the forward substitution y = L^-1 P rhs rides along: the lane that owns a row keeps its partial
//                        y in a register (the next row of that lane, 64 further, in a second one, fetched 64 columns ahead), the
//                        finished y_j is broadcast by v_readlane and the column is applied as an axpy.
//   band_solve_kernel    both substitutions on Lb, gather and scatter through perm inside the kernel: y_j and then x_j live at
//                        x[perm[j]], so x may alias rhs.  Column oriented, columns of Lb fetched two chunks of eight ahead.
//   band_backward_kernel x = P^T L^-T y for a y in banded order.  Also column oriented (an axpy with ROW j of L, a strided read of
//                        Lb that does not sit on the dependent chain), because a wave-wide reduction per column would put six
//                        dependent cross-lane steps between x_j and x_j-1; the chain here is a division, a readlane and an fma.
//                        x aliasing y: x is first written in banded order over y, then permuted through the wave's LDS.
// A pivot that is not positive is replaced by one and the item goes on (info = banded column + 1, first such), as
// thx_chol_factor finishes a failed item.  Every element of Lb, y, x and info is written; nothing is accumulated in memory: the
// result is independent of what the buffers held and the same from run to run.  Accumulation in the working dtype (as pbtrf).
#include "common.cuh"

namespace thx {

constexpr int BAND_MAX_KD = THX_BAND_MAX_KD;
constexpr int BAND_CH = 8;                 // columns gathered / fetched per chunk
constexpr int BAND_WAVES = 4;              // problems per workgroup at most
constexpr size_t BAND_LDS_BUDGET = 65536;  // dynamic LDS per workgroup

static_assert(BAND_MAX_KD == 63, "one row per lane: the window has at most 64 rows");

__device__ __forceinline__ float lane_bcast(float x, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
__device__ __forceinline__ double lane_bcast(double x, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
  return __hiloint2double(hi, lo);
}

// LDS elements of one wave of the factorisation: the window's sums, two chunks of H's band, the finished column
__host__ __device__ inline size_t band_wave_elems(int w, int S) { return (size_t)(w + 2 * BAND_CH) * S + 64; }

// the wave's own LDS writes become visible to its reads.  LDS only ("local"): a fence over every address space also orders the
// column's store to Lb and the band columns in flight
__device__ __forceinline__ void band_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
}

template <typename T>
__global__ __launch_bounds__(64 * BAND_WAVES) void band_factor_kernel(const T* __restrict__ H, int64_t ld, int n, int kd, int B,
                                                                      const int32_t* __restrict__ perm,
                                                                      const T* __restrict__ damping, int ellipsoidal, T eps,
                                                                      T* __restrict__ Lb, int32_t* __restrict__ info,
                                                                      const T* __restrict__ rhs, T* __restrict__ y, int64_t ldv,
                                                                      int S) {
  extern __shared__ __attribute__((aligned(16))) char band_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x >> 6) + wave;
  if (b >= B) return;
  const int w = kd + 1;
  T* acc = reinterpret_cast<T*>(band_smem) + (size_t)wave * band_wave_elems(w, S);   // w slots: the sums of the window's columns
  T* raw = acc + w * S;                                                               // 2 CH slots: columns of H's band
  T* lcol = raw + 2 * BAND_CH * S;                                                    // 64: the finished column
  const T* Hb = H + (int64_t)b * ld * ld;
  T* Lo = Lb + (int64_t)b * n * w;
  const bool damp = damping != nullptr;
  const T lam = damp ? damping[b] : T(0);

  // elements (c + lane, c) of the permuted band for the CH columns from c0 on (zero outside the matrix), damped
  auto load_chunk = [&](int c0, T(&pre)[BAND_CH]) {   // (every load at a clamped address, selected afterwards: no load waits
    int pc[BAND_CH], pr[BAND_CH];                      //  behind a branch, the sixteen of a chunk are in flight together)
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      pc[cc] = perm[min(c0 + cc, n - 1)];
      pr[cc] = perm[min(c0 + cc + lane, n - 1)];
    }
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) pre[cc] = Hb[(int64_t)max(pc[cc], pr[cc]) * ld + min(pc[cc], pr[cc])];
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      T v = pre[cc];
      const T dv = ellipsoidal ? v + (lam * v + eps) : v + lam;
      v = (lane == 0 && damp) ? dv : v;
      pre[cc] = (lane <= kd && c0 + cc + lane < n) ? v : T(0);
    }
  };
  auto store_chunk = [&](int c0, const T(&pre)[BAND_CH]) {   // (c0 a multiple of CH: slots c0 mod 2 CH ..)
    const int slot = c0 & BAND_CH;
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc)
      if (lane <= kd) raw[(slot + cc) * S + lane] = pre[cc];
  };

  T pre[BAND_CH];
  load_chunk(0, pre);
  store_chunk(0, pre);
  load_chunk(BAND_CH, pre);
  for (int k = lane; k < w * S; k += 64) acc[k] = T(0);

  // fused forward substitution: the partial y of this lane's row inside the window, and of its next row
  const bool fwd = rhs != nullptr;
  const T* rb = fwd ? rhs + (int64_t)b * ldv : nullptr;
  T ycur = T(0), ynext = T(0), yout = T(0), fcur = T(0), fnext = T(0);
  // rhs of the row that enters at column j (row j + 128): lane cc of a chunk fetches it one chunk ahead, v_readlane hands it over
  auto fetch_rows = [&](int r0) {
    const int r = r0 + lane;
    const T v = rb[perm[min(r, n - 1)]];
    return (lane < BAND_CH && r < n) ? v : T(0);
  };
  if (fwd) {
    if (lane < n) ycur = rb[perm[lane]];
    if (lane + 64 < n) ynext = rb[perm[lane + 64]];
    fcur = fetch_rows(128);
  }

  // this lane's first element of the update rectangle: (p0, q) = (lane / w, lane mod w), then 64 further every step
  const int P = w / 2, dp = 64 / w, dq = 64 % w;
  const int p_first = lane / w, q_first = lane % w;

  int bad = 0, jm = 0;   // jm = j mod w
  for (int j0 = 0; j0 < n; j0 += BAND_CH) {
    store_chunk(j0 + BAND_CH, pre);       // the next chunk's columns, over the slots of the previous chunk
    load_chunk(j0 + 2 * BAND_CH, pre);    // (in flight while this chunk is factorised)
    if (fwd) fnext = fetch_rows(j0 + BAND_CH + 128);
    band_lds_fence();
    const int jend = min(j0 + BAND_CH, n);
    for (int j = j0; j < jend; ++j) {
      T* sum = acc + jm * S;
      const T* col = raw + (j & (2 * BAND_CH - 1)) * S;
      T d = col[0] - sum[0];
      if (!(d > T(0))) {
        if (bad == 0) bad = j + 1;
        d = T(1);
      }
      const T dr = sqrt(d), isq = T(1) / dr;
      const int i = (lane - j) & 63;   // this lane owns row j + i
      T v = T(0);
      if (i <= kd) {
        v = i == 0 ? dr : (col[i] - sum[i]) * isq;
        sum[i] = T(0);                 // the slot is column j + kd + 1's from the next step on
        lcol[i] = v;
        Lo[(int64_t)j * w + i] = v;
      }
      if (fwd) {
        const T yj = lane_bcast(ycur / v, j & 63);
        if (i >= 1 && i <= kd) ycur = fma(-v, yj, ycur);
        const T enters = lane_bcast(fcur, j - j0);
        if (i == 0) {
          yout = yj;
          ycur = ynext;
          ynext = enters;
        }
        if ((j & 63) == 63 || j == n - 1) {
          const int r = (j & ~63) + lane;
          if (r <= j) y[(int64_t)b * ldv + r] = yout;
        }
      }
      band_lds_fence();
      // sums(j + i, j + a) += l_i l_a for 1 <= a <= i <= kd
      int p0 = p_first, q = q_first;
      while (p0 < P) {
        const int p = p0 + 1;
        int ri, ca;
        bool valid = true;
        if (q < p) {
          ri = p;
          ca = q + 1;
        } else {
          ri = w - p;
          ca = q - p + 1;
          valid = ri != p;   // (kd odd: the middle row is paired with itself)
        }
        if (valid) {
          int cs = jm + ca;
          cs = cs >= w ? cs - w : cs;
          T* e = acc + cs * S + (ri - ca);
          *e = fma(lcol[ri], lcol[ca], *e);
        }
        q += dq;
        p0 += dp;
        if (q >= w) {
          q -= w;
          ++p0;
        }
      }
      band_lds_fence();
      jm = jm + 1 == w ? 0 : jm + 1;
    }
    fcur = fnext;
  }
  if (lane == 0) info[b] = bad;
}

// ---- substitutions on Lb ------------------------------------------------------------------------------------------------------
// columns j0 .. j0 + CH - 1 of Lb as the forward substitution reads them: element (j + i, j) for the lane that owns row j + i
template <typename T>
__device__ __forceinline__ void band_cols_fwd(const T* __restrict__ Lo, int n, int kd, int j0, int lane, T (&c)[BAND_CH]) {
#pragma unroll
  for (int cc = 0; cc < BAND_CH; ++cc) {
    const int j = j0 + cc, i = (lane - j) & 63;
    const bool valid = j < n && i <= kd;
    const T v = Lo[valid ? (int64_t)j * (kd + 1) + i : 0];   // (a clamped address and a select: no load waits behind a branch)
    c[cc] = valid ? v : T(0);
  }
}

// rows jt, jt - 1, .. of L as the backward substitution reads them: element (j, j - i) for the lane that owns row j - i
template <typename T>
__device__ __forceinline__ void band_rows_bwd(const T* __restrict__ Lo, int kd, int jt, int lane, T (&c)[BAND_CH]) {
#pragma unroll
  for (int cc = 0; cc < BAND_CH; ++cc) {
    const int j = jt - cc, i = (j - lane) & 63, r = j - i;
    const bool valid = j >= 0 && i <= kd && r >= 0;
    const T v = Lo[valid ? (int64_t)r * (kd + 1) + i : 0];
    c[cc] = valid ? v : T(0);
  }
}

// y = L^-1 P src, y_j stored at dst[perm[j]] (dst may be src: position perm[j] is read before it is written, by the same lane)
template <typename T>
__device__ __forceinline__ void band_forward(const T* __restrict__ Lo, int n, int kd, const int32_t* __restrict__ perm, const T* src,
                                             T* dst, int lane) {
  T ycur = T(0), ynext = T(0);
  int pcur = 0, pnext = 0;
  if (lane < n) {
    pcur = perm[lane];
    ycur = src[pcur];
  }
  if (lane + 64 < n) {
    pnext = perm[lane + 64];
    ynext = src[pnext];
  }
  // the row that enters at column j (row j + 128): lane cc of a chunk fetches it one chunk ahead, v_readlane hands it over
  T fcur, fnext;
  int qcur, qnext;
  auto fetch_rows = [&](int r0, T& f, int& q) {
    const int r = r0 + lane;
    q = perm[min(r, n - 1)];
    const T v = src[q];
    f = (lane < BAND_CH && r < n) ? v : T(0);
  };
  fetch_rows(128, fcur, qcur);
  T cur[BAND_CH], nxt[BAND_CH], nx2[BAND_CH];   // (fetched two chunks ahead of the chunk being applied)
  band_cols_fwd(Lo, n, kd, 0, lane, cur);
  band_cols_fwd(Lo, n, kd, BAND_CH, lane, nxt);
  for (int j0 = 0; j0 < n; j0 += BAND_CH) {
    band_cols_fwd(Lo, n, kd, j0 + 2 * BAND_CH, lane, nx2);
    fetch_rows(j0 + BAND_CH + 128, fnext, qnext);
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      const int j = j0 + cc;
      if (j < n) {
        const int i = (lane - j) & 63;
        const T v = cur[cc];
        const T yj = lane_bcast(ycur / v, j & 63);
        if (i >= 1 && i <= kd) ycur = fma(-v, yj, ycur);
        const T enters = lane_bcast(fcur, cc);
        const int enters_at = __builtin_amdgcn_readlane(qcur, cc);
        if (i == 0) {
          dst[pcur] = yj;
          ycur = ynext;
          pcur = pnext;
          ynext = enters;
          pnext = enters_at;
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      cur[cc] = nxt[cc];
      nxt[cc] = nx2[cc];
    }
    fcur = fnext;
    qcur = qnext;
  }
}

// x = L^-T y.  YPERM: y_j is read at src[perm[j]], else at src[j]; SCATTER: x_j is written at dst[perm[j]] (the linearization's
// order), else at dst[j].  dst may be src when both use the same position (a row's position is read before it is written).
template <typename T, bool YPERM, bool SCATTER>
__device__ __forceinline__ void band_backward(const T* __restrict__ Lo, int n, int kd, const int32_t* __restrict__ perm, const T* src,
                                              T* dst, int lane) {
  T ycur = T(0), ynext = T(0);
  int pcur = 0, pnext = 0;
  const int r0 = n - 1 - ((n - 1 - lane) & 63);   // this lane's last row
  if (r0 >= 0) {
    if (YPERM || SCATTER) pcur = perm[r0];
    ycur = src[YPERM ? pcur : r0];
  }
  if (r0 - 64 >= 0) {
    if (YPERM || SCATTER) pnext = perm[r0 - 64];
    ynext = src[YPERM ? pnext : r0 - 64];
  }
  // the row that enters at column j (row j - 128): lane cc of a chunk fetches it one chunk ahead, v_readlane hands it over
  T fcur, fnext;
  int qcur = 0, qnext = 0;
  auto fetch_rows = [&](int r0, T& f, int& q) {   // rows r0, r0 - 1, ..
    const int r = r0 - lane, rc = max(r, 0);
    if (YPERM || SCATTER) q = perm[rc];
    const T v = src[YPERM ? q : rc];
    f = (lane < BAND_CH && r >= 0) ? v : T(0);
  };
  fetch_rows(n - 1 - 128, fcur, qcur);
  T cur[BAND_CH], nxt[BAND_CH], nx2[BAND_CH];   // (fetched two chunks ahead of the chunk being applied)
  band_rows_bwd(Lo, kd, n - 1, lane, cur);
  band_rows_bwd(Lo, kd, n - 1 - BAND_CH, lane, nxt);
  for (int jt = n - 1; jt >= 0; jt -= BAND_CH) {
    band_rows_bwd(Lo, kd, jt - 2 * BAND_CH, lane, nx2);
    fetch_rows(jt - BAND_CH - 128, fnext, qnext);
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      const int j = jt - cc;
      if (j >= 0) {
        const int i = (j - lane) & 63;
        const T v = cur[cc];
        const T xj = lane_bcast(ycur / v, j & 63);
        if (i >= 1 && i <= kd) ycur = fma(-v, xj, ycur);
        const T enters = lane_bcast(fcur, cc);
        const int enters_at = __builtin_amdgcn_readlane(qcur, cc);
        if (i == 0) {
          dst[SCATTER ? pcur : j] = xj;
          ycur = ynext;
          pcur = pnext;
          ynext = enters;
          pnext = enters_at;
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < BAND_CH; ++cc) {
      cur[cc] = nxt[cc];
      nxt[cc] = nx2[cc];
    }
    fcur = fnext;
    qcur = qnext;
  }
}

template <typename T>
__global__ __launch_bounds__(64 * BAND_WAVES) void band_solve_kernel(const T* __restrict__ Lb, int n, int kd, int B,
                                                                     const int32_t* __restrict__ perm, const T* rhs, T* x,
                                                                     int64_t ldv) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  const T* Lo = Lb + (int64_t)b * n * (kd + 1);
  T* xb = x + (int64_t)b * ldv;
  band_forward<T>(Lo, n, kd, perm, rhs + (int64_t)b * ldv, xb, lane);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");   // the y other lanes of this wave wrote
  __builtin_amdgcn_wave_barrier();
  band_backward<T, true, true>(Lo, n, kd, perm, xb, xb, lane);
}

// INPLACE: x is y's buffer -- x in banded order over y, then x[perm[k]] = x[k] through LDS (n elements, one wave per workgroup)
template <typename T, bool INPLACE>
__global__ __launch_bounds__(64 * BAND_WAVES) void band_backward_kernel(const T* __restrict__ Lb, int n, int kd, int B,
                                                                        const int32_t* __restrict__ perm, const T* y, T* x,
                                                                        int64_t ldv) {
  extern __shared__ __attribute__((aligned(16))) char band_smem[];
  const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= B) return;
  const T* Lo = Lb + (int64_t)b * n * (kd + 1);
  T* xb = x + (int64_t)b * ldv;
  if constexpr (!INPLACE) {
    band_backward<T, false, true>(Lo, n, kd, perm, y + (int64_t)b * ldv, xb, lane);
  } else {
    T* stage = reinterpret_cast<T*>(band_smem);
    band_backward<T, false, false>(Lo, n, kd, perm, xb, xb, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < n; k += 64) stage[k] = xb[k];
    band_lds_fence();
    for (int k = lane; k < n; k += 64) xb[perm[k]] = stage[k];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int check_band_sizes(const char* who, int n, int kd, int B) {
  if (n <= 0 || B <= 0) return fail(who, ": need n > 0, B > 0");
  if (kd < 0 || kd >= n) return fail(who, ": need 0 <= kd < n");
  if (kd > BAND_MAX_KD) {
    const std::string msg = ": kd above the limit of " + std::to_string(BAND_MAX_KD) + " of the banded solver (one window row per lane)";
    return fail(who, msg.c_str());
  }
  return 0;
}

template <typename T>
int band_factor_impl(const void* H, int64_t ld, int n, int kd, int B, const int32_t* perm, const void* damping, int ellipsoidal,
                     double eps, void* Lb, int32_t* info, const void* rhs, void* y, int64_t ldv, hipStream_t st) {
  const int w = kd + 1, S = w | 1;
  const size_t per_wave = band_wave_elems(w, S) * sizeof(T);
  int waves = (int)(BAND_LDS_BUDGET / per_wave);
  waves = waves < 1 ? 1 : (waves > BAND_WAVES ? BAND_WAVES : waves);
  const unsigned grid = (unsigned)((B + waves - 1) / waves);
  band_factor_kernel<T><<<dim3(grid), dim3(64 * waves), per_wave * waves, st>>>(
      static_cast<const T*>(H), ld, n, kd, B, perm, static_cast<const T*>(damping), ellipsoidal, (T)eps, static_cast<T*>(Lb), info,
      static_cast<const T*>(rhs), static_cast<T*>(y), ldv, S);
  return check_launch("thx_band_factor");
}

template <typename T>
int band_solve_impl(const void* Lb, int n, int kd, int B, const int32_t* perm, const void* rhs, void* x, int64_t ldv, bool forward,
                    hipStream_t st) {
  const T* L = static_cast<const T*>(Lb);
  const T* in = static_cast<const T*>(rhs);
  T* out = static_cast<T*>(x);
  const unsigned grid = (unsigned)((B + BAND_WAVES - 1) / BAND_WAVES);
  if (forward) {
    band_solve_kernel<T><<<dim3(grid), dim3(64 * BAND_WAVES), 0, st>>>(L, n, kd, B, perm, in, out, ldv);
    return check_launch("thx_band_solve");
  }
  if (rhs != x) {
    band_backward_kernel<T, false><<<dim3(grid), dim3(64 * BAND_WAVES), 0, st>>>(L, n, kd, B, perm, in, out, ldv);
  } else {
    const size_t lds = (size_t)n * sizeof(T);
    if (lds > BAND_LDS_BUDGET)
      return fail("thx_band_solve_backward: x may alias y only up to 64 KB of y per problem (it is permuted through LDS)");
    band_backward_kernel<T, true><<<dim3((unsigned)B), dim3(64), lds, st>>>(L, n, kd, B, perm, in, out, ldv);
  }
  return check_launch("thx_band_solve_backward");
}

static int band_solve_dispatch(const char* who, const void* Lb, int n, int kd, int B, const int32_t* perm, const void* rhs, void* x,
                               int64_t ldv, bool forward, int dtype, void* stream) {
  if (!Lb || !perm || !rhs || !x) return fail(who, ": null pointer");
  if (int r = check_band_sizes(who, n, kd, B)) return r;
  if (ldv < n) return fail(who, ": ldv < n");
  THX_DISPATCH(dtype, return band_solve_impl<float>(Lb, n, kd, B, perm, rhs, x, ldv, forward, as_stream(stream)),
               return band_solve_impl<double>(Lb, n, kd, B, perm, rhs, x, ldv, forward, as_stream(stream)));
  return 0;
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_band_factor(const void* H, int64_t ld, int32_t n, int32_t kd, int32_t B, const int32_t* perm, const void* damping,
                    int ellipsoidal, double damping_eps, void* Lb, int32_t* info, const void* rhs, void* y, int64_t ldv, int dtype,
                    void* stream) {
  if (!H || !perm || !Lb || !info || (rhs != nullptr) != (y != nullptr)) return fail("thx_band_factor: null pointer");
  if (int r = check_band_sizes("thx_band_factor", n, kd, B)) return r;
  if (ld < n) return fail("thx_band_factor: ld < n");
  if (rhs && ldv < n) return fail("thx_band_factor: ldv < n");
  if (H == Lb) return fail("thx_band_factor: Lb must not alias H (the source stays undamped)");
  if (rhs && rhs == y) return fail("thx_band_factor: y must not alias rhs (rhs is read in another order than y is written)");
  THX_DISPATCH(dtype,
               return band_factor_impl<float>(H, ld, n, kd, B, perm, damping, ellipsoidal, damping_eps, Lb, info, rhs, y, ldv,
                                              as_stream(stream)),
               return band_factor_impl<double>(H, ld, n, kd, B, perm, damping, ellipsoidal, damping_eps, Lb, info, rhs, y, ldv,
                                               as_stream(stream)));
  return 0;
}

int thx_band_solve(const void* Lb, int32_t n, int32_t kd, int32_t B, const int32_t* perm, const void* rhs, void* x, int64_t ldv,
                   int dtype, void* stream) {
  return band_solve_dispatch("thx_band_solve", Lb, n, kd, B, perm, rhs, x, ldv, true, dtype, stream);
}

int thx_band_solve_backward(const void* Lb, int32_t n, int32_t kd, int32_t B, const int32_t* perm, const void* y, void* x,
                            int64_t ldv, int dtype, void* stream) {
  return band_solve_dispatch("thx_band_solve_backward", Lb, n, kd, B, perm, y, x, ldv, false, dtype, stream);
}

}  // extern "C"
