// thx_homog_vjp, the backward of the homography family's implicit step (the forward: homog_kernels.hip; shared: homog_family.cuh).
// A source of its own so that it alone is built without packed fp32 arithmetic (theseus_amd/build.py) and the forward's code stays
// what it was.
#pragma clang fp contract(off)
#include "homog_family.cuh"

namespace thx {

// ---- thx_homog_vjp: the gradient of psi = u^T g, g = -sum_t J_t^T e_t at a detached state, w.r.t. the auxiliary tensors ----------
// floor(), the clamping, the mask m and the count N = C sum m are constants, as in the torch class.  For an alignment term with
// weight w, err = sum m d^2 / N and A = J_raw . u_t = (2 / N) sum m d S, S = alpha dsx + beta dsy (alpha, beta: the directional
// derivatives of ix, iy along u_t): psi = -w^2 A err.  With c1 = -2 w^2 err / N and c2 = -2 w^2 A / N
//   d psi / d dst[c, p]      = -m (c1 S + c2 d)
//   d psi / d src[c, cell_k] += m (c1 (S om_k + d (alpha d om_k / d ix + beta d om_k / d iy)) + c2 d om_k),  om_k the corner's weight
//   d psi / d w              = -2 w A err
// A prior term: psi = -sum_i u_i w_i^2 (x_i - t_i).
// Stage 1: homog_partial_kernel (the ten sums), then homog_vjp_terms_kernel: one thread per (term, problem) writes the record.
// Stage 2: homog_vjp_pixels_kernel, below.  Stage 3: vjp_reduce_kernel of term_family.cuh on the record.
constexpr int kVjpRec = THX_HOMOG_REC;
constexpr int kVjpSlice = THX_HOMOG_VJP_SLICE;                // channels per workgroup of stage 2
constexpr int kVjpPix = THX_HOMOG_CHUNK / kHomogThreads;      // pixels per thread and chunk
constexpr int kVjpKeys = 4 * THX_HOMOG_CHUNK;                 // (cell, slot) keys per chunk: four corners per pixel
constexpr int kVjpSeg = kVjpKeys / kHomogThreads;             // sorted positions per thread
constexpr int kVjpSlotBits = 12;
constexpr unsigned kVjpPad = ~0u;                             // sorts last; its cell, 2^20 - 1, is no cell of a map the host accepts
static_assert(kVjpKeys == 1 << kVjpSlotBits && kVjpKeys == kVjpSeg * kHomogThreads && THX_HOMOG_MAX_CELLS == 1 << (32 - kVjpSlotBits),
              "key layout");

// record of an alignment term: 0 d psi / d w, 1 c1, 2 c2; of a prior: 0-7 d psi / d target, 8-15 d psi / d weight (wdim = 1: the
// sum in 8).  Terms that thx_homog_eval skips write zeros.
template <typename T>
__global__ void __launch_bounds__(256)
homog_vjp_terms_kernel(const thx_homog_term* __restrict__ terms, int n_terms, int n_align, const T* __restrict__ x, int64_t ldx, int n,
                       const T* __restrict__ u, int64_t ldu, int m, int64_t j_total, const double* __restrict__ scratch, int chunks,
                       double* __restrict__ rec, int B) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)n_terms * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  const thx_homog_term& tm = terms[t];
  double o[kVjpRec];
#pragma unroll
  for (int k = 0; k < kVjpRec; ++k) o[k] = 0.0;
  const int dim = tm.kind == THX_HOMOG_ALIGN ? 1 : 8;
  const bool placed = !(tm.row0 < 0 || tm.row0 + dim > m || tm.j_off < 0 || tm.j_off + (int64_t)8 * dim > j_total);
  if (placed && tm.kind == THX_HOMOG_ALIGN && t < n_align && homog_align_ok(tm, n)) {
    double sums[THX_HOMOG_SUMS];
    homog_sum_chunks<THX_HOMOG_SUMS>(scratch, tm, t, b, B, chunks, sums);
    const double w = (double)aux_at<T>(tm, 2, b), N = sums[1], err = sums[0] / N;
    double A = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) A += -(2.0 * sums[2 + k] / N) * (double)u[(int64_t)b * ldu + tm.col[0] + k];
    o[0] = -2.0 * w * A * err;
    o[1] = -2.0 * w * w * err / N;
    o[2] = -2.0 * w * w * A / N;
  } else if (placed && tm.kind != THX_HOMOG_ALIGN && homog_prior_ok(tm, n)) {
    double gw = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double w = (double)aux_at<T>(tm, 1, b, tm.wdim == 8 ? i : 0), ui = (double)u[(int64_t)b * ldu + tm.col[0] + i];
      const double gi = -2.0 * ui * w * ((double)x[(int64_t)b * ldx + tm.col[0] + i] - (double)aux_at<T>(tm, 0, b, i));
      o[i] = ui * w * w;
      if (tm.wdim == 8) o[8 + i] = gi;
      else gw += gi;
    }
    if (tm.wdim != 8) o[8] = gw;
  }
#pragma unroll
  for (int k = 0; k < kVjpRec; ++k) rec[((int64_t)t * kVjpRec + k) * B + b] = o[k];
}

// position i of the sorted values in LDS: one pad per thread's segment, so that the threads' walks fall into different banks
__device__ __forceinline__ int vjp_at(int i) { return i + (i >> 4); }

// Stage 2, the pixel pass: one workgroup per (alignment term, problem, slice of kVjpSlice channels) walks the chunks of
// THX_HOMOG_CHUNK destination pixels in index order.  A thread owns pixels tid, tid + 256, ... of the chunk and keeps their geometry
// (weights, alpha, beta, the four cells) in registers for all channels of the slice.
//   grad feat_dst: one writer per element, coalesced.
//   grad feat_src: the chunk's 4096 keys cell * 4096 + slot (slot = 4 * pixel + corner; they do not depend on the channel) are
//   sorted once by a bitonic network in LDS; pos[slot] is where the slot's value goes.  Per channel every thread places its 16
//   values, then walks ITS 16 consecutive sorted positions: a run of equal cells that lies inside the walk is added to
//   grad_src[b, c, cell] at once; the open ends go through a segmented scan over the 256 threads (shuffles inside a wave, the four
//   waves in index order), so a border cell's run of thousands costs the same tree as any other.  Every run has one writer, the
//   workgroup owns its (problem, channels) and takes the chunks in order behind barriers: plain read-modify-write, no atomics, the
//   same bits on every call.
template <typename T>
__global__ void __launch_bounds__(kHomogThreads)
homog_vjp_pixels_kernel(const thx_homog_term* __restrict__ terms, int n_align, const T* __restrict__ x, int64_t ldx, int n,
                        const T* __restrict__ u, int64_t ldu, const double* __restrict__ rec, const int64_t* __restrict__ map_off,
                        T* __restrict__ out, int64_t out_elems, int slices, int B) {
  __shared__ unsigned key[kVjpKeys];
  __shared__ unsigned short pos[kVjpKeys];
  __shared__ double val[kVjpKeys + kHomogThreads];
  __shared__ double wave_v[kHomogWaves];
  __shared__ int wave_f[kHomogWaves];
  const int64_t wg = blockIdx.x;
  const int slice = (int)(wg % slices), b = (int)((wg / slices) % B), t = (int)(wg / ((int64_t)slices * B));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (t >= n_align) return;
  // (everything up to the chunk loop is uniform over the workgroup)
  const thx_homog_term& tm = terms[t];
  if (!homog_align_ok(tm, n)) return;
  const int Hh = tm.rows, Ww = tm.cols, C = tm.chans;
  const int64_t P = (int64_t)Hh * Ww;
  const int c_begin = slice * kVjpSlice, c_end = c_begin + kVjpSlice < C ? c_begin + kVjpSlice : C;
  if (P >= THX_HOMOG_MAX_CELLS || c_begin >= C) return;
  const int64_t per = (int64_t)C * P, o_src = map_off[2 * t], o_dst = map_off[2 * t + 1];
  T* __restrict__ gs = (o_src >= 0 && o_src + per * B <= out_elems) ? out + o_src + per * b : nullptr;
  T* __restrict__ gd = (o_dst >= 0 && o_dst + per * B <= out_elems) ? out + o_dst + per * b : nullptr;
  if (!gs && !gd) return;
  const T* __restrict__ src = static_cast<const T*>(tm.aux[0]) + (int64_t)b * tm.aux_bstride[0];
  const T* __restrict__ dst = static_cast<const T*>(tm.aux[1]) + (int64_t)b * tm.aux_bstride[1];
  const double c1 = rec[((int64_t)t * kVjpRec + 1) * B + b], c2 = rec[((int64_t)t * kVjpRec + 2) * B + b];
  T h[8], G[9];
  double U[9];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    h[k] = x[(int64_t)b * ldx + tm.col[0] + k];
    U[k] = (double)u[(int64_t)b * ldu + tm.col[0] + k];
  }
  U[8] = 0.0;
  homog_inverse<T>(h, G);
  const double half_w = 0.5 * (double)(Ww - 1), half_h = 0.5 * (double)(Hh - 1);
  // Sorted positions that hold a pad key (pixels past the map or outside the mask) are not placed in that chunk: they keep zero or
  // a finite value of an earlier chunk or channel.  They form the last run, whose cell is kPadCell, and every add below skips
  // that cell (``cl``, ``cell_in``, ``cell_last``): those three tests are what keeps the stale values out of the gradient.
  for (int i = tid; i < kVjpKeys + kHomogThreads; i += kHomogThreads) val[i] = 0.0;

  for (int64_t p0 = 0; p0 < P; p0 += THX_HOMOG_CHUNK) {
    // the geometry of this thread's pixels; live: inside the map and the mask
    double wx1[kVjpPix], wx0[kVjpPix], wy1[kVjpPix], wy0[kVjpPix], al[kVjpPix], be[kVjpPix];
    int cell[kVjpPix][4], at[kVjpPix][4];
    bool live[kVjpPix];
#pragma unroll
    for (int r = 0; r < kVjpPix; ++r) {
      const int64_t pix = p0 + (int64_t)r * kHomogThreads + tid;
      live[r] = false;
      if (pix < P) {
        HomogPixel<T> g;
        homog_pixel<T>(G, Hh, Ww, pix, g);
        live[r] = g.mask;
        wx1[r] = (double)g.wx1, wx0[r] = (double)g.wx0, wy1[r] = (double)g.wy1, wy0[r] = (double)g.wy0;
        // alpha = D ix, beta = D iy along u_t: D q = -G (U q) from d q / d H_kl = -G[:, k] q_l, then the quotient rule
        const double q[3] = {(double)g.q0, (double)g.q1, (double)g.q2};
        double z[3], dq[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) z[k] = (U[3 * k] * q[0] + U[3 * k + 1] * q[1]) + U[3 * k + 2] * q[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) dq[k] = -(((double)G[3 * k] * z[0] + (double)G[3 * k + 1] * z[1]) + (double)G[3 * k + 2] * z[2]);
        al[r] = (dq[0] - (double)g.u * dq[2]) / q[2] * half_w;
        be[r] = (dq[1] - (double)g.v * dq[2]) / q[2] * half_h;
#pragma unroll
        for (int k = 0; k < 4; ++k) cell[r][k] = (int)g.cell[k];
      }
      if (!live[r]) {
        wx1[r] = wx0[r] = wy1[r] = wy0[r] = al[r] = be[r] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) cell[r][k] = 0;
      }
    }
    unsigned heads = 0;            // bit j: sorted position kVjpSeg * tid + j starts a run of equal cells
    unsigned cell_in = 0, cell_last = 0;   // the cells of the run that enters this thread's walk and of the chunk's last run
    if (gs) {
      __syncthreads();   // (the previous chunk's walks have read key)
#pragma unroll
      for (int r = 0; r < kVjpPix; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned slot = (unsigned)((r * kHomogThreads + tid) * 4 + k);
          key[slot] = live[r] ? ((unsigned)cell[r][k] << kVjpSlotBits) | slot : kVjpPad;
        }
      __syncthreads();
      for (int k = 2; k <= kVjpKeys; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int p = tid; p < kVjpKeys / 2; p += kHomogThreads) {   // pair p of this step: (i, i + j), bit j of i clear
            const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
            const unsigned a = key[i], c = key[l];
            if ((a > c) == ((i & k) == 0)) key[i] = c, key[l] = a;
          }
          __syncthreads();
        }
      for (int i = tid; i < kVjpKeys; i += kHomogThreads) {
        const unsigned a = key[i];
        if (a != kVjpPad) pos[a & (kVjpKeys - 1)] = (unsigned short)i;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < kVjpPix; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) at[r][k] = live[r] ? vjp_at(pos[(r * kHomogThreads + tid) * 4 + k]) : 0;
      unsigned prev = tid > 0 ? key[kVjpSeg * tid - 1] >> kVjpSlotBits : kVjpPad;   // (position 0 is a head)
      cell_in = prev, cell_last = key[kVjpKeys - 1] >> kVjpSlotBits;
#pragma unroll
      for (int j = 0; j < kVjpSeg; ++j) {
        const unsigned cur = key[kVjpSeg * tid + j] >> kVjpSlotBits;
        if (j == 0 ? (tid == 0 || cur != prev) : cur != prev) heads |= 1u << j;
        prev = cur;
      }
    }
    constexpr unsigned kPadCell = kVjpPad >> kVjpSlotBits;
    for (int c = c_begin; c < c_end; ++c) {
      const T* __restrict__ sc = src + (int64_t)c * P;
#pragma unroll
      for (int r = 0; r < kVjpPix; ++r) {
        if (!live[r]) continue;
        const int64_t pix = p0 + (int64_t)r * kHomogThreads + tid;
        const double vnw = (double)sc[cell[r][0]], vne = (double)sc[cell[r][1]], vsw = (double)sc[cell[r][2]],
                     vse = (double)sc[cell[r][3]];
        const double nw = wx1[r] * wy1[r], ne = wx0[r] * wy1[r], sw = wx1[r] * wy0[r], se = wx0[r] * wy0[r];
        const double d = (((vnw * nw + vne * ne) + vsw * sw) + vse * se) - (double)dst[(int64_t)c * P + pix];
        const double dsx = (vne - vnw) * wy1[r] + (vse - vsw) * wy0[r], dsy = (vsw - vnw) * wx1[r] + (vse - vne) * wx0[r];
        const double S = al[r] * dsx + be[r] * dsy;
        if (gd) gd[(int64_t)c * P + pix] = (T)(-(c1 * S + c2 * d));
        if (gs) {
          const double a = c1 * S + c2 * d, e = c1 * d;   // value_k = a om_k + e (alpha d om_k / d ix + beta d om_k / d iy)
          val[at[r][0]] = a * nw + e * (-al[r] * wy1[r] - be[r] * wx1[r]);
          val[at[r][1]] = a * ne + e * (al[r] * wy1[r] - be[r] * wx0[r]);
          val[at[r][2]] = a * sw + e * (-al[r] * wy0[r] + be[r] * wx1[r]);
          val[at[r][3]] = a * se + e * (al[r] * wy0[r] + be[r] * wx0[r]);
        }
      }
      if (!gs) continue;
      T* __restrict__ gc = gs + (int64_t)c * P;
      __syncthreads();
      // this thread's walk: ``acc`` is the open run; ``seen``: a head lies in the walk
      double acc = 0.0, pre = 0.0;
      bool seen = false;
#pragma unroll
      for (int j = 0; j < kVjpSeg; ++j) {
        const int i = kVjpSeg * tid + j;
        const double v = val[vjp_at(i)];
        if (heads >> j & 1u) {
          if (seen) {   // the run before this head began and ended inside the walk
            const unsigned cl = key[i - 1] >> kVjpSlotBits;
            if (cl != kPadCell) gc[cl] = (T)((double)gc[cl] + acc);
          } else {
            pre = acc;
          }
          seen = true;
          acc = v;
        } else {
          acc += v;
        }
      }
      // segmented inclusive scan of (seen, acc) over the threads: lanes by __shfl_up, then the waves in index order
      double sv = acc;
      int sf = seen ? 1 : 0;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double pv = __shfl_up(sv, off, 64);
        const int pf = __shfl_up(sf, off, 64);
        if (lane >= off) {
          if (!sf) sv += pv;
          sf |= pf;
        }
      }
      if (lane == 63) wave_v[wave] = sv, wave_f[wave] = sf;
      __syncthreads();
      double carry = 0.0;
      for (int w = 0; w < wave; ++w) carry = wave_f[w] ? wave_v[w] : carry + wave_v[w];
      const double incl = sf ? sv : carry + sv;
      double excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = carry;
      // the run that enters the walk ends at its first head; the chunk's last run ends with the last thread
      if (seen && tid > 0 && cell_in != kPadCell) gc[cell_in] = (T)((double)gc[cell_in] + (excl + pre));
      if (tid == kHomogThreads - 1 && cell_last != kPadCell) gc[cell_last] = (T)((double)gc[cell_last] + (seen ? acc : excl + acc));
    }
  }
}

}  // namespace thx

using namespace thx;

extern "C" int thx_homog_vjp(const thx_homog_term* terms, int32_t n_terms, int32_t n_align, const void* x, int64_t ldx, int32_t n,
                             const void* u, int64_t ldu, int32_t m, int64_t j_total, void* scratch, int32_t chunks, double* rec,
                             const thx_homog_grad_plan* plan, void* grad_out, int32_t B, int dtype, void* stream) {
  const char* who = "thx_homog_vjp";
  unsigned partial = 0;
  if (int rc = family_check(who, !u || !scratch || !rec || !plan || !grad_out, terms, n_terms, x, 1, B, dtype,
                            homog_bad_size(ldx, n, n_terms, n_align, chunks)))
    return rc;
  if (ldu < n) return fail(who, ": ldu < n");
  if (m < 1 || j_total < 8) return fail(who, ": m < 1 or j_total < 8");
  const thx_homog_grad_plan p = *plan;
  if (p.n_tensors < 0 || p.n_pairs < 0 || p.n_maps < 0 || p.max_cells < 0 || p.max_chans < 0 || p.out_elems < 1)
    return fail(who, ": negative size in the plan");
  if ((p.n_tensors > 0 && (!p.tensors || !p.pairs)) || (p.n_maps > 0 && !p.map_off)) return fail(who, ": null pointer in the plan");
  if (p.n_maps > 0 && (p.n_maps != n_align || p.max_cells < 4 || p.max_chans < 1))
    return fail(who, ": the plan's maps do not fit the alignment terms");
  if (p.n_maps > 0 && p.max_cells >= THX_HOMOG_MAX_CELLS)
    return fail(who, ": a feature map of 2^20 or more pixels does not fit the 32-bit sort keys of the feat_src scatter");
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  auto at = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  if (at(u) % el || at(grad_out) % el || at(rec) % 8 || at(p.tensors) % 8 || at(p.pairs) % 4 || at(p.map_off) % 8)
    return fail(who, ": pointer not aligned");
  if (int rc = homog_check_partial(who, scratch, n_align, B, chunks, &partial)) return rc;
  const int64_t term_blocks = ((int64_t)n_terms * B + 255) / 256, slices = (p.max_chans + kVjpSlice - 1) / kVjpSlice;
  if (term_blocks > (int64_t)INT32_MAX || (int64_t)p.n_tensors * B > (int64_t)INT32_MAX ||
      (int64_t)n_align * B * slices > (int64_t)INT32_MAX)
    return fail(who, ": grid limit exceeded (n_terms * B, tensors * B or n_align * B * channel slices)");
  hipStream_t s = as_stream(stream);
  const dim3 block(256), pblock(kHomogThreads);
  double* sc = static_cast<double*>(scratch);
  if (int rc = homog_launch_partial(who, terms, n_align, x, ldx, n, sc, chunks, partial, B, dtype, s)) return rc;
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(homog_vjp_terms_kernel<float>, dim3((unsigned)term_blocks), block, 0, s, terms, n_terms, n_align,
                                  (const float*)x, ldx, n, (const float*)u, ldu, m, j_total, (const double*)sc, chunks, rec, B),
               hipLaunchKernelGGL(homog_vjp_terms_kernel<double>, dim3((unsigned)term_blocks), block, 0, s, terms, n_terms, n_align,
                                  (const double*)x, ldx, n, (const double*)u, ldu, m, j_total, (const double*)sc, chunks, rec, B));
  if (p.n_maps > 0) {
    const dim3 grid((unsigned)((int64_t)n_align * B * slices));
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL(homog_vjp_pixels_kernel<float>, grid, pblock, 0, s, terms, n_align, (const float*)x, ldx, n,
                                    (const float*)u, ldu, (const double*)rec, p.map_off, (float*)grad_out, p.out_elems, (int)slices, B),
                 hipLaunchKernelGGL(homog_vjp_pixels_kernel<double>, grid, pblock, 0, s, terms, n_align, (const double*)x, ldx, n,
                                    (const double*)u, ldu, (const double*)rec, p.map_off, (double*)grad_out, p.out_elems, (int)slices,
                                    B));
  }
  if (p.n_tensors > 0) {
    const dim3 grid((unsigned)((int64_t)p.n_tensors * B));
    THX_DISPATCH(dtype,
                 hipLaunchKernelGGL((vjp_reduce_kernel<float, kVjpRec>), grid, block, 0, s, (const double*)rec, n_terms, p.tensors,
                                    p.pairs, p.n_pairs, (float*)grad_out, p.out_elems, B),
                 hipLaunchKernelGGL((vjp_reduce_kernel<double, kVjpRec>), grid, block, 0, s, (const double*)rec, n_terms, p.tensors,
                                    p.pairs, p.n_pairs, (double*)grad_out, p.out_elems, B));
  }
  return check_launch(who);
}
