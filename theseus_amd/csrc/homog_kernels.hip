// Homography image alignment, dense Lucas-Kanade (examples/homography_estimation.py of the reference): the cost family of the
// example's objective -- the masked mean squared difference between a feature map warped by H = [h0 .. h7, 1] and a second one
// (homography_error_fn over theseus/third_party/utils.py grid_sample) and Difference priors on the 8-dof variable
// (theseus/embodied/misc/local_cost_fn.py:16-75).  The torch twin is theseus_amd/embodied.py: HomographyAlignment; the
// per-pixel arithmetic below follows it operation for operation.
//
// Both exports are two launches.
// (a) homog_partial_kernel: one 256-thread workgroup per (alignment term, problem, chunk of THX_HOMOG_CHUNK destination pixels).
//     A thread takes pixels tid, tid + 256, ... of the chunk (feat_dst is read coalesced), computes the pixel's source point, the
//     four bilinear weights and the four clamped corner offsets ONCE, then loops over the channels: four gathers from feat_src, one
//     coalesced load from feat_dst.  It accumulates sum m d^2, sum m and -- eval only -- the eight sums of m d ds/dh in fp64
//     registers; the workgroup reduces them by a fixed-order tree (__shfl_down inside a wave, then the four waves through LDS) into
//     scratch (n_align, B, chunks, THX_HOMOG_SUMS).  No atomics: two calls give the same bits.
// (b) homog_finish_eval_kernel: one thread per (term, problem), as in the other families: an alignment term adds its chunks in
//     index order and writes the weighted 1 x 8 block and error; a prior term is evaluated here.
//     homog_finish_error_kernel: one workgroup per problem; thread i sums the squares of terms i, i + 256, ... in fp64, then the
//     fixed-order tree of term_family.cuh.
//
// Per-pixel arithmetic runs in the run's dtype with contraction off, so floor() and the mask test see the values the torch class
// computes.  Registers: 20 for the fp64 accumulators of the eval stage; LDS: 4 x 10 doubles.
#pragma clang fp contract(off)
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

// the alignment term reads inside the state and its sizes are usable
__device__ __forceinline__ bool homog_align_ok(const thx_homog_term& tm, int n) {
  return tm.kind == THX_HOMOG_ALIGN && tm.col[0] >= 0 && tm.col[0] + 8 <= n && tm.rows >= 2 && tm.cols >= 2 && tm.chans >= 1;
}

__device__ __forceinline__ int homog_term_chunks(const thx_homog_term& tm, int chunks) {
  const int64_t own = ((int64_t)tm.rows * tm.cols + THX_HOMOG_CHUNK - 1) / THX_HOMOG_CHUNK;
  return own < (int64_t)chunks ? (int)own : chunks;
}

// acc[0 .. NS) of the workgroup's threads -> out[0 .. NS): lanes by __shfl_down, waves in index order
template <int NS>
__device__ __forceinline__ void homog_reduce_store(const double* acc, double* __restrict__ out) {
  __shared__ double part[kHomogWaves][NS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    double v = acc[s];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][s] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    double v = part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kHomogWaves; ++w) v += part[w][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

template <typename T, bool JAC>
__global__ void __launch_bounds__(kHomogThreads)
homog_partial_kernel(const thx_homog_term* __restrict__ terms, int n_align, const T* __restrict__ x, int64_t ldx, int n,
                     double* __restrict__ scratch, int chunks, int B) {
  constexpr int NS = JAC ? THX_HOMOG_SUMS : 2;
  const int64_t wg = blockIdx.x;
  const int chunk = (int)(wg % chunks), b = (int)((wg / chunks) % B), t = (int)(wg / ((int64_t)chunks * B));
  if (t >= n_align) return;   // (never: the grid is n_align * B * chunks)
  const thx_homog_term& tm = terms[t];   // (read in place: a private copy of the 128 bytes would live in scratch)
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  const int Hh = tm.rows, Ww = tm.cols, C = tm.chans;
  const int64_t P = (int64_t)Hh * Ww, p0 = (int64_t)chunk * THX_HOMOG_CHUNK;
  if (homog_align_ok(tm, n) && p0 < P) {   // (uniform over the workgroup)
    const T* __restrict__ src = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
    const T* __restrict__ dst = static_cast<const T*>(tm.aux[1]) + (int64_t)b * tm.aux_bstride[1];
    T h[8], G[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = x[(int64_t)b * ldx + tm.col[0] + k];
    homog_inverse<T>(h, G);
    const T wm1 = (T)(Ww - 1), hm1 = (T)(Hh - 1);
    for (int r = 0; r < THX_HOMOG_CHUNK / kHomogThreads; ++r) {
      const int64_t pix = p0 + (int64_t)r * kHomogThreads + threadIdx.x;
      if (pix >= P) break;
      const int i = (int)(pix / Ww), j = (int)(pix % Ww);
      // destination pixel -> source point
      const T px = (T)(2 * j) / wm1 - (T)1, py = (T)(2 * i) / hm1 - (T)1;
      const T q0 = (G[0] * px + G[1] * py) + G[2], q1 = (G[3] * px + G[4] * py) + G[5], q2 = (G[6] * px + G[7] * py) + G[8];
      const T u = q0 / q2, v = q1 / q2;
      const T ix = ((u + (T)1) / (T)2) * wm1, iy = ((v + (T)1) / (T)2) * hm1;
      const T x0 = floor(ix), y0 = floor(iy), x1 = x0 + (T)1, y1 = y0 + (T)1;
      // bilinear weights from the unclamped corners (utils.py:25-28)
      const T wx1 = x1 - ix, wx0 = ix - x0, wy1 = y1 - iy, wy0 = iy - y0;
      const T nw = wx1 * wy1, ne = wx0 * wy1, sw = wx1 * wy0, se = wx0 * wy0;
      if (!((((nw + ne) + sw) + se) > (T)0.9)) continue;   // the mask (also NaN)
      const int xi0 = homog_idx(x0, Ww - 1), xi1 = homog_idx(x1, Ww - 1), yi0 = homog_idx(y0, Hh - 1), yi1 = homog_idx(y1, Hh - 1);
      const int64_t onw = (int64_t)yi0 * Ww + xi0, one = (int64_t)yi0 * Ww + xi1, osw = (int64_t)yi1 * Ww + xi0,
                    ose = (int64_t)yi1 * Ww + xi1;
      double sse = 0.0, A = 0.0, Bv = 0.0;
      for (int c = 0; c < C; ++c) {
        const T* __restrict__ sc = src + (int64_t)c * P;
        const T vnw = sc[onw], vne = sc[one], vsw = sc[osw], vse = sc[ose];
        const T s = ((vnw * nw + vne * ne) + vsw * sw) + vse * se;
        const T d = s - dst[(int64_t)c * P + pix];
        sse += (double)(d * d);
        if (JAC) {
          const T dsx = (vne - vnw) * wy1 + (vse - vsw) * wy0, dsy = (vsw - vnw) * wx1 + (vse - vne) * wx0;
          A += (double)(d * dsx);
          Bv += (double)(d * dsy);
        }
      }
      acc[0] += sse;
      acc[1] += (double)C;   // (the mask has the feature maps' shape: every channel counts)
      if (JAC) {
        // d s / d h_(3k+l) = -(G^T r)_k q_l,  r = d s / d q  (d q / d H_kl = -G[:, k] q_l)
        const T gu = (T)A * (wm1 / (T)2), gv = (T)Bv * (hm1 / (T)2);
        const T r0 = gu / q2, r1 = gv / q2, r2 = -(gu * u + gv * v) / q2;
        const T q[3] = {q0, q1, q2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const T tk = (G[k] * r0 + G[3 + k] * r1) + G[6 + k] * r2;
#pragma unroll
          for (int l = 0; l < 3; ++l)
            if (3 * k + l < 8) acc[2 + 3 * k + l] += (double)(tk * q[l]);
        }
      }
    }
  }
  homog_reduce_store<NS>(acc, scratch + (((int64_t)t * B + b) * chunks + chunk) * THX_HOMOG_SUMS);
}

// Difference on an 8-dof Euclidean variable: e = (x - target) * w, J = diag(w)
template <typename T>
__device__ __forceinline__ void homog_prior(const thx_homog_term& tm, const T* __restrict__ xb, int b, T* __restrict__ e,
                                            T* __restrict__ J) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const T w = aux_at<T>(tm, 1, b, tm.wdim == 8 ? i : 0);
    e[i] = (xb[tm.col[0] + i] - aux_at<T>(tm, 0, b, i)) * w;
    if (J) {
#pragma unroll
      for (int k = 0; k < 8; ++k) J[8 * i + k] = i == k ? w : (T)0;
    }
  }
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

// the weighted error of an alignment term from its two sums
template <typename T>
__device__ __forceinline__ T homog_align_error(const thx_homog_term& tm, int b, const double* sums) {
  return (T)((double)aux_at<T>(tm, 2, b) * (sums[0] / sums[1]));
}

template <typename T>
__global__ void __launch_bounds__(256)
homog_finish_eval_kernel(const thx_homog_term* __restrict__ terms, int n_terms, int n_align, const T* __restrict__ x, int64_t ldx,
                         int n, const double* __restrict__ scratch, int chunks, T* __restrict__ J, int64_t j_total,
                         T* __restrict__ e, int64_t lde, int m, int B) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_homog_term& tm = terms[t];
  const int dim = tm.kind == THX_HOMOG_ALIGN ? 1 : 8;
  if (tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)8 * dim > j_total) return;
  T* eb = e + (int64_t)b * lde + tm.row0;
  T* Jb = J + tm.j_off * B + (int64_t)8 * dim * b;
  if (tm.kind == THX_HOMOG_ALIGN) {
    if (t >= n_align || !homog_align_ok(tm, n)) return;
    double sums[THX_HOMOG_SUMS];
    homog_sum_chunks<THX_HOMOG_SUMS>(scratch, tm, t, b, B, chunks, sums);
    const double w = (double)aux_at<T>(tm, 2, b);
    eb[0] = homog_align_error<T>(tm, b, sums);
#pragma unroll
    for (int k = 0; k < 8; ++k) Jb[k] = (T)(-(2.0 * sums[2 + k] / sums[1]) * w);
  } else {
    if (!homog_prior_ok(tm, n)) return;
    T ev[8];
    homog_prior<T>(tm, x + (int64_t)b * ldx, b, ev, Jb);
#pragma unroll
    for (int i = 0; i < 8; ++i) eb[i] = ev[i];
  }
}

template <typename T>
__global__ void __launch_bounds__(kErrThreads)
homog_finish_error_kernel(const thx_homog_term* __restrict__ terms, int n_terms, int n_align, const T* __restrict__ x, int64_t ldx,
                          int n, const double* __restrict__ scratch, int chunks, T* __restrict__ err, int B) {
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < n_terms; t += kErrThreads) {
    const thx_homog_term& tm = terms[t];
    if (tm.kind == THX_HOMOG_ALIGN) {
      if (t >= n_align || !homog_align_ok(tm, n)) continue;
      double sums[2];
      homog_sum_chunks<2>(scratch, tm, t, b, B, chunks, sums);
      const double v = (double)homog_align_error<T>(tm, b, sums);
      acc += v * v;
    } else {
      if (!homog_prior_ok(tm, n)) continue;
      T ev[8];
      homog_prior<T>(tm, x + (int64_t)b * ldx, b, ev, nullptr);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += (double)ev[i] * (double)ev[i];
    }
  }
  store_half_sum(acc, err + b);
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

}  // namespace thx

using namespace thx;

extern "C" int thx_homog_eval(const thx_homog_term* terms, int32_t n_terms, int32_t n_align, const void* x, int64_t ldx, int32_t n,
                              void* scratch, int32_t chunks, void* J, int64_t j_total, void* e, int64_t lde, int32_t m, int32_t B,
                              int dtype, void* stream) {
  const char* who = "thx_homog_eval";
  unsigned blocks = 0, partial = 0;
  if (int rc = family_check(who, !J || !e || !scratch, terms, n_terms, x, 1, B, dtype, homog_bad_size(ldx, n, n_terms, n_align, chunks)))
    return rc;
  if (int rc = family_check_eval(who, J, j_total < 8 ? ": j_total < 8" : nullptr, e, lde, m, n_terms, B, dtype, &blocks)) return rc;
  if (int rc = homog_check_partial(who, scratch, n_align, B, chunks, &partial)) return rc;
  const dim3 pgrid(partial), pblock(kHomogThreads), grid(blocks), block(256);
  double* sc = static_cast<double*>(scratch);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL((homog_partial_kernel<float, true>), pgrid, pblock, 0, as_stream(stream), terms, n_align,
                                  (const float*)x, ldx, n, sc, chunks, B),
               hipLaunchKernelGGL((homog_partial_kernel<double, true>), pgrid, pblock, 0, as_stream(stream), terms, n_align,
                                  (const double*)x, ldx, n, sc, chunks, B));
  if (int rc = check_launch(who)) return rc;
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(homog_finish_eval_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, n_align,
                                  (const float*)x, ldx, n, (const double*)sc, chunks, (float*)J, j_total, (float*)e, lde, m, B),
               hipLaunchKernelGGL(homog_finish_eval_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, n_align,
                                  (const double*)x, ldx, n, (const double*)sc, chunks, (double*)J, j_total, (double*)e, lde, m, B));
  return check_launch(who);
}

extern "C" int thx_homog_error(const thx_homog_term* terms, int32_t n_terms, int32_t n_align, const void* x, int64_t ldx, int32_t n,
                               void* scratch, int32_t chunks, void* err, int32_t B, int dtype, void* stream) {
  const char* who = "thx_homog_error";
  unsigned partial = 0;
  if (int rc = family_check(who, !err || !scratch, terms, n_terms, x, 1, B, dtype, homog_bad_size(ldx, n, n_terms, n_align, chunks)))
    return rc;
  if (reinterpret_cast<uintptr_t>(err) % (dtype == THX_F32 ? 4 : 8)) return fail(who, ": pointer not aligned");
  if (int rc = homog_check_partial(who, scratch, n_align, B, chunks, &partial)) return rc;
  const dim3 pgrid(partial), pblock(kHomogThreads), grid((unsigned)B), block(kErrThreads);   // (B <= INT32_MAX)
  double* sc = static_cast<double*>(scratch);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL((homog_partial_kernel<float, false>), pgrid, pblock, 0, as_stream(stream), terms, n_align,
                                  (const float*)x, ldx, n, sc, chunks, B),
               hipLaunchKernelGGL((homog_partial_kernel<double, false>), pgrid, pblock, 0, as_stream(stream), terms, n_align,
                                  (const double*)x, ldx, n, sc, chunks, B));
  if (int rc = check_launch(who)) return rc;
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(homog_finish_error_kernel<float>, grid, block, 0, as_stream(stream), terms, n_terms, n_align,
                                  (const float*)x, ldx, n, (const double*)sc, chunks, (float*)err, B),
               hipLaunchKernelGGL(homog_finish_error_kernel<double>, grid, block, 0, as_stream(stream), terms, n_terms, n_align,
                                  (const double*)x, ldx, n, (const double*)sc, chunks, (double*)err, B));
  return check_launch(who);
}
