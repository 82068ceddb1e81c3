// What the homography family's two sources share (homog_kernels.hip: thx_homog_eval, thx_homog_error; homog_vjp_kernels.hip:
// thx_homog_vjp): the pixel geometry, the term guards, the chunk sums and the host checks.  The including source sets
// ``#pragma clang fp contract(off)`` first: the per-pixel arithmetic runs in the run's dtype with contraction off.
#pragma once
#include "term_family.cuh"

namespace thx {

constexpr int kHomogThreads = 256;
constexpr int kHomogWaves = kHomogThreads / 64;

// the clamped index of a floor()ed coordinate (the clamp is applied before the conversion: no out-of-range conversion, NaN -> 0)
template <typename T>
__device__ __forceinline__ int homog_idx(T v, int hi) {
  if (!(v > (T)0)) return 0;
  return v < (T)hi ? (int)v : hi;
}

// G = adj(H) / det(H), H = [h0 .. h7, 1] row major, by the cofactor formula (HomographyAlignment._inverse)
template <typename T>
__device__ __forceinline__ void homog_inverse(const T* __restrict__ h, T* __restrict__ G) {
  const T a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7], i = (T)1;
  const T A[9] = {e * i - f * k, c * k - b * i, b * f - c * e,
                  f * g - d * i, a * i - c * g, c * d - a * f,
                  d * k - e * g, b * g - a * k, a * e - b * d};
  const T det = (a * A[0] + b * A[3]) + c * A[6];
#pragma unroll
  for (int n = 0; n < 9; ++n) G[n] = A[n] / det;
}

// One destination pixel's geometry, shared by the forward and the backward so that every floor() and the mask land in the same
// place: pixel -> source point (q, u, v, ix, iy), the bilinear weights from the UNCLAMPED corners (utils.py:25-28), the mask and the
// four clamped cells (nw, ne, sw, se) as offsets into one channel.  Runs in the run's dtype with contraction off.
template <typename T>
struct HomogPixel {
  T q0, q1, q2, u, v, ix, iy, wx1, wx0, wy1, wy0, nw, ne, sw, se;
  int64_t cell[4];
  bool mask;
};

template <typename T>
__device__ __forceinline__ void homog_pixel(const T* __restrict__ G, int Hh, int Ww, int64_t pix, HomogPixel<T>& g) {
  const T wm1 = (T)(Ww - 1), hm1 = (T)(Hh - 1);
  const int i = (int)(pix / Ww), j = (int)(pix % Ww);
  const T px = (T)(2 * j) / wm1 - (T)1, py = (T)(2 * i) / hm1 - (T)1;
  g.q0 = (G[0] * px + G[1] * py) + G[2], g.q1 = (G[3] * px + G[4] * py) + G[5], g.q2 = (G[6] * px + G[7] * py) + G[8];
  g.u = g.q0 / g.q2, g.v = g.q1 / g.q2;
  g.ix = ((g.u + (T)1) / (T)2) * wm1, g.iy = ((g.v + (T)1) / (T)2) * hm1;
  const T x0 = floor(g.ix), y0 = floor(g.iy), x1 = x0 + (T)1, y1 = y0 + (T)1;
  g.wx1 = x1 - g.ix, g.wx0 = g.ix - x0, g.wy1 = y1 - g.iy, g.wy0 = g.iy - y0;
  g.nw = g.wx1 * g.wy1, g.ne = g.wx0 * g.wy1, g.sw = g.wx1 * g.wy0, g.se = g.wx0 * g.wy0;
  g.mask = (((g.nw + g.ne) + g.sw) + g.se) > (T)0.9;
  const int xi0 = homog_idx(x0, Ww - 1), xi1 = homog_idx(x1, Ww - 1), yi0 = homog_idx(y0, Hh - 1), yi1 = homog_idx(y1, Hh - 1);
  g.cell[0] = (int64_t)yi0 * Ww + xi0, g.cell[1] = (int64_t)yi0 * Ww + xi1;
  g.cell[2] = (int64_t)yi1 * Ww + xi0, g.cell[3] = (int64_t)yi1 * Ww + xi1;
}

// the alignment term reads inside the state and its sizes are usable
__device__ __forceinline__ bool homog_align_ok(const thx_homog_term& tm, int n) {
  return tm.kind == THX_HOMOG_ALIGN && tm.col[0] >= 0 && tm.col[0] + 8 <= n && tm.rows >= 2 && tm.cols >= 2 && tm.chans >= 1;
}

__device__ __forceinline__ int homog_term_chunks(const thx_homog_term& tm, int chunks) {
  const int64_t own = ((int64_t)tm.rows * tm.cols + THX_HOMOG_CHUNK - 1) / THX_HOMOG_CHUNK;
  return own < (int64_t)chunks ? (int)own : chunks;
}

__device__ __forceinline__ bool homog_prior_ok(const thx_homog_term& tm, int n) {
  return tm.kind == THX_HOMOG_PRIOR && tm.col[0] >= 0 && tm.col[0] + 8 <= n && (tm.wdim == 1 || tm.wdim == 8);
}

// the chunks of alignment term t, problem b, added in index order -> sums[0 .. NS)
template <int NS>
__device__ __forceinline__ void homog_sum_chunks(const double* __restrict__ scratch, const thx_homog_term& tm, int t, int b, int B,
                                                 int chunks, double* sums) {
  const double* p = scratch + ((int64_t)t * B + b) * chunks * THX_HOMOG_SUMS;
  const int own = homog_term_chunks(tm, chunks);
#pragma unroll
  for (int s = 0; s < NS; ++s) sums[s] = 0.0;
  for (int c = 0; c < own; ++c)
#pragma unroll
    for (int s = 0; s < NS; ++s) sums[s] += p[(int64_t)c * THX_HOMOG_SUMS + s];
}

// the family's own size checks: the message of the first that fails
inline const char* homog_bad_size(int64_t ldx, int32_t n, int32_t n_terms, int32_t n_align, int32_t chunks) {
  if (n < 8) return ": n < 8";
  if (ldx < n) return ": ldx < n";
  if (n_align < 1 || n_align > n_terms) return ": n_align outside 1 ... n_terms";
  if (chunks < 1) return ": chunks < 1";
  return nullptr;
}

// ... and what both exports check after family_check: the scratch's alignment, the grid of stage (a) -> ``blocks``
inline int homog_check_partial(const char* who, const void* scratch, int32_t n_align, int32_t B, int32_t chunks, unsigned* blocks) {
  if (reinterpret_cast<uintptr_t>(scratch) % 8) return fail(who, ": pointer not aligned");
  const int64_t ab = (int64_t)n_align * B;   // (< 2^62)
  if (ab > (int64_t)INT32_MAX || ab * chunks > (int64_t)INT32_MAX) return fail(who, ": grid limit exceeded (n_align * B * chunks)");
  *blocks = (unsigned)(ab * chunks);
  return 0;
}

// stage (a) of thx_homog_eval on `stream` (homog_kernels.hip): the ten sums per (alignment term, problem, chunk) into scratch
int homog_launch_partial(const char* who, const thx_homog_term* terms, int32_t n_align, const void* x, int64_t ldx, int32_t n,
                         double* scratch, int32_t chunks, unsigned blocks, int32_t B, int dtype, hipStream_t stream);

}  // namespace thx
