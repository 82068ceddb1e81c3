// The DCEM-specific part of one iteration of the differentiable cross-entropy method (theseus/optimizer/nonlinear/dcem.py:94-158;
// theseus/third_party/lml.py:53-177) and its backward: thx_dcem_update, thx_dcem_update_vjp (include/theseus_hip.h).
//
// One workgroup of 256 threads per problem.  Per problem the work is S values of fX, a few thousand sigmoids and S x n
// multiply-adds: everything but X itself lives in LDS or registers, there is no host decision (the reference's bracketing loop
// ends every round in one) and no MFMA.  Elementwise values are formed in the run's dtype; every sum is accumulated in fp64 in
// a FIXED order (a lane's strided elements, a shuffle tree inside the wave, the waves in order): no atomics, two calls give the
// same bits.  Standardising, the softmax and the moments run on fp64 values throughout, so an fp32 output is rounded once; the
// sigmoids of the LML rounds -- the bulk -- are the run's dtype.
//
// LDS plan.  thx_dcem_update: xs[S] in the run's dtype (the standardised scores, then the weights) -- S <= THX_DCEM_MAX_S = 4096,
// 32 KB in fp64 -- + 256 doubles of partial sums + 256 flags: below 36 KB, so four workgroups fit a CU beside each other and
// no attribute is needed for the dynamic part.  thx_dcem_update_vjp: gw[S] doubles (dL/dw, then dL/dx), the partial sums and
// the factors of 256 columns at a time: 40 KB at the limit.
// The N-th / N+1-th largest score is found by rank counting (S^2 / 256 compares per thread, LDS broadcast reads): exact, no
// sort network, ties broken by the lower sample index; 4096 is also where that quadratic stops being negligible.
#include <cmath>

#include "common.cuh"

namespace thx {

constexpr int kDcemThreads = 256;
constexpr int kDcemWaves = kDcemThreads / 64;

enum { kDcemHard = 0, kDcemSoftmax = 1, kDcemLml = 2 };

inline int dcem_mode(double temp, int32_t n_elite) {
  if (!(temp < INFINITY)) return kDcemHard;   // (dcem.py:117: temp None / inf -- NaN goes the same way there)
  return n_elite == 1 ? kDcemSoftmax : kDcemLml;
}

template <typename T>
__device__ __forceinline__ T dcem_sigmoid(T v) {
  return (T)1 / ((T)1 + exp(-v));
}

// sum over the workgroup, every thread gets it: lane partials by a shuffle tree, then the four waves in order
__device__ __forceinline__ double dcem_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;   // (lane 0 holds the wave's sum)
}

__device__ __forceinline__ double dcem_block_sum(double v, double* __restrict__ red) {
  v = dcem_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int k = 1; k < kDcemWaves; ++k) s += red[k];
  __syncthreads();
  return s;
}

__device__ __forceinline__ double dcem_block_max(double v, double* __restrict__ red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int k = 1; k < kDcemWaves; ++k) s = fmax(s, red[k]);
  __syncthreads();
  return s;
}

// mean and unbiased std of problem b's fX (dcem.py:119-121), kept in fp64: the scores are rounded to the run's dtype once
template <typename T>
__device__ __forceinline__ void dcem_standardise(const T* __restrict__ fX, int S, int B, int b, double* __restrict__ red, double& mean,
                                                 double& stdv) {
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < S; i += kDcemThreads) acc += (double)fX[(int64_t)i * B + b];
  mean = dcem_block_sum(acc, red) / (double)S;
  acc = 0.0;
  for (int i = t; i < S; i += kDcemThreads) {
    const double d = (double)fX[(int64_t)i * B + b] - mean;
    acc += d * d;
  }
  stdv = sqrt(dcem_block_sum(acc, red) / (double)(S - 1));   // (S == 1: 0 / 0 = NaN, as torch.std)
}

template <typename T>
__global__ void __launch_bounds__(kDcemThreads)
dcem_update_kernel(const T* __restrict__ fX, const T* __restrict__ X, int S, int B, int n, int n_elite, T temp, int normalize,
                   T lml_eps, int lml_n_iter, int branch, int mode, T* __restrict__ mu, T* __restrict__ sigma, T* __restrict__ w,
                   T* __restrict__ nu_out, T* __restrict__ bracket, int32_t* __restrict__ flags) {
  extern __shared__ double dcem_lds[];
  double* __restrict__ red = dcem_lds;                                     // 256 partial sums
  int* __restrict__ neg = reinterpret_cast<int*>(dcem_lds + kDcemThreads);   // 256 flags (grid value < 0) + 2 selected indices
  T* __restrict__ xs = reinterpret_cast<T*>(dcem_lds + kDcemThreads + kDcemThreads / 2 + 2);
  const int t = threadIdx.x, b = blockIdx.x;
  const double N = (double)n_elite;
  T nu = (T)0, lo = (T)0, hi = (T)0;
  int flag = 0;
  if (t < 2) neg[kDcemThreads + t] = 0;   // (scores that are NaN have no rank: the selected indices stay inside xs)

  // ---- 1. the scores: x = -temp * standardised fX (hard mode ranks the raw fX) ----
  if (mode == kDcemHard) {
    for (int i = t; i < S; i += kDcemThreads) xs[i] = fX[(int64_t)i * B + b];
  } else {
    double mean = 0.0, inv = 1.0;
    if (normalize) {
      double stdv;
      dcem_standardise<T>(fX, S, B, b, red, mean, stdv);
      inv = stdv + 1e-6;
    }
    for (int i = t; i < S; i += kDcemThreads) {
      double f = (double)fX[(int64_t)i * B + b];
      if (normalize) f = (f - mean) / inv;
      xs[i] = (T)(-f * (double)temp);
    }
  }
  __syncthreads();

  // ---- 2. the weights ----
  if (mode == kDcemHard) {
    // weight 1 for the n_elite smallest fX, ties to the lower sample index (dcem.py:136-140)
    // (parked in the output while the others still read the scores; a thread reads back only what it wrote itself)
    T* __restrict__ wb = w + (int64_t)b * S;
    for (int i = t; i < S; i += kDcemThreads) {
      const T v = xs[i];
      int rank = 0;
      for (int j = 0; j < S; ++j) {
        const T u = xs[j];
        rank += (u < v) || (u == v && j < i);
      }
      wb[i] = rank < n_elite ? (T)1 : (T)0;
    }
    __syncthreads();
    for (int i = t; i < S; i += kDcemThreads) xs[i] = wb[i];
  } else if (mode == kDcemSoftmax) {
    double m = -INFINITY;
    for (int i = t; i < S; i += kDcemThreads) m = fmax(m, (double)xs[i]);
    const double mx = dcem_block_max(m, red);
    double acc = 0.0;
    for (int i = t; i < S; i += kDcemThreads) acc += exp((double)xs[i] - mx);
    const double tot = dcem_block_sum(acc, red);
    for (int i = t; i < S; i += kDcemThreads) xs[i] = (T)(exp((double)xs[i] - mx) / tot);   // (each weight rounded once)
  } else if (S <= n_elite) {
    for (int i = t; i < S; i += kDcemThreads) xs[i] = (T)(1.0 - 1e-5);   // lml.py:76-77
  } else {
    // the bracket: the N-th and N+1-th largest score, widened by the interval the sigmoid saturates on (lml.py:88-92)
    for (int i = t; i < S; i += kDcemThreads) {
      const T v = xs[i];
      int rank = 0;
      for (int j = 0; j < S; ++j) {
        const T u = xs[j];
        rank += (u > v) || (u == v && j < i);
      }
      if (rank == n_elite - 1) neg[kDcemThreads] = i;
      if (rank == n_elite) neg[kDcemThreads + 1] = i;
    }
    __syncthreads();
    lo = -xs[neg[kDcemThreads]] - (T)7;
    hi = -xs[neg[kDcemThreads + 1]] + (T)7;
    __syncthreads();
    // rounds of `branch` grid values each (lml.py:94-122); P threads share one grid point, K points per pass
    const int P = branch >= kDcemThreads ? 1 : kDcemThreads / branch;
    const int K = kDcemThreads / P;
    const int kk = t / P, jj = t % P;
    const T step = (T)1 / (T)(branch - 1);   // torch.linspace(0, 1, branch): from the start below the middle, from the end above
    auto grid = [&](int k, T l, T h) -> T {
      const T ls = k < branch / 2 ? step * (T)k : (T)1 - step * (T)(branch - k - 1);
      return (h - l) * ls + l;
    };
    int it = 0;
    for (; it < lml_n_iter; ++it) {
      if (!(hi - lo > lml_eps)) break;
      int count = 0;
      for (int k0 = 0; k0 < branch; k0 += K) {
        const int k = k0 + kk;
        double acc = 0.0;
        if (kk < K && k < branch) {
          const T nk = grid(k, lo, hi);
          for (int i = jj; i < S; i += P) acc += (double)dcem_sigmoid<T>(xs[i] + nk);
        }
        red[t] = acc;
        __syncthreads();
        if (jj == 0 && kk < K && k < branch) {
          double fs = red[t];
          for (int q = 1; q < P; ++q) fs += red[t + q];
          neg[kk] = (T)(fs - N) < (T)0;
        }
        __syncthreads();
        const int here = branch - k0 < K ? branch - k0 : K;
        for (int q = 0; q < here; ++q) count += neg[q];
        __syncthreads();
      }
      int i_lower = count - 1;
      if (i_lower > branch - 2) i_lower = branch - 2;
      T widen = (T)0;
      if (i_lower < 0) {
        // every grid value non-negative: the reference warns and means to restart 7 below (its own indexing there is broken)
        flag |= THX_DCEM_FLAG_ALL_NONNEG;
        i_lower = 0;
        widen = (T)7;
      }
      const T nl = grid(i_lower, lo, hi), nh = grid(i_lower + 1, lo, hi);
      lo = nl - widen;
      hi = nh;
    }
    if (hi - lo > lml_eps) flag |= THX_DCEM_FLAG_NOT_CONVERGED;
    nu = lo + (hi - lo) / (T)2;
    for (int i = t; i < S; i += kDcemThreads) xs[i] = dcem_sigmoid<T>(xs[i] + nu);
  }
  __syncthreads();
  for (int i = t; i < S; i += kDcemThreads) w[(int64_t)b * S + i] = xs[i];
  if (t == 0) {
    nu_out[b] = nu;
    bracket[2 * (int64_t)b] = lo;
    bracket[2 * (int64_t)b + 1] = hi;
    flags[b] = flag;
  }

  // ---- 3. the moments: mu = sum w X / N, sigma = sqrt(sum w (X - mu)^2 / N) [+ 1e-10 in hard mode] (dcem.py:149-154).
  //      C columns per pass, G groups of samples per column; the groups' partials are added in order ----
  const int C = n < kDcemThreads ? n : kDcemThreads;
  const int G = kDcemThreads / C;
  const int c = t % C, g = t / C;
  const double hard_eps = mode == kDcemHard ? 1e-10 : 0.0;
  for (int j0 = 0; j0 < n; j0 += C) {
    const int j = j0 + c;
    const bool on = g < G && j < n;
    double acc = 0.0;
    if (on)
      for (int i = g; i < S; i += G) acc += (double)xs[i] * (double)X[((int64_t)i * B + b) * n + j];
    red[t] = acc;
    __syncthreads();
    double m = 0.0;
    if (on) {
      for (int q = 0; q < G; ++q) m += red[q * C + c];
      m = (double)(T)(m / N);
    }
    __syncthreads();
    acc = 0.0;
    if (on)
      for (int i = g; i < S; i += G) {
        const double d = (double)X[((int64_t)i * B + b) * n + j] - m;
        acc += (double)xs[i] * d * d;
      }
    red[t] = acc;
    __syncthreads();
    if (on && g == 0) {
      double v = 0.0;
      for (int q = 0; q < G; ++q) v += red[q * C + c];
      mu[(int64_t)b * n + j] = (T)m;
      sigma[(int64_t)b * n + j] = (T)(sqrt(v / N) + (double)hard_eps);
    }
    __syncthreads();
  }
}

// Backward.  With W = sum w, d_ij = X_ij - mu_j, v_j = (sigma_j - hard_eps)^2:
//   gv_j  = grad_sigma_j / (2 sqrt(v_j))
//   gmt_j = grad_mu_j - 2 gv_j mu_j (N - W) / N          (d v / d mu does not vanish: sum_i w_i d_ij = mu_j (N - W))
//   grad_X_ij = w_i (gmt_j + 2 gv_j d_ij) / N
//   grad_w_i  = sum_j (gmt_j X_ij + gv_j d_ij^2) / N
// then the weights' backward (LML: lml.py:169-171; softmax; nothing in hard mode) and the standardisation's.
template <typename T>
__global__ void __launch_bounds__(kDcemThreads)
dcem_update_vjp_kernel(const T* __restrict__ grad_mu, const T* __restrict__ grad_sigma, const T* __restrict__ X,
                       const T* __restrict__ fX, const T* __restrict__ w, const T* __restrict__ mu, const T* __restrict__ sigma, int S,
                       int B, int n, int n_elite, T temp, int normalize, int mode, T* __restrict__ grad_X, T* __restrict__ grad_fX) {
  extern __shared__ double dcem_lds[];
  double* __restrict__ red = dcem_lds;
  double* __restrict__ col_m = dcem_lds + kDcemThreads;   // the factors of a chunk of 256 columns
  double* __restrict__ col_gv = col_m + kDcemThreads;
  double* __restrict__ col_gmt = col_gv + kDcemThreads;
  double* __restrict__ gw = col_gmt + kDcemThreads;      // (S) dL/dw_i, then dL/dx_i
  const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
  const double N = (double)n_elite;
  const T* __restrict__ wb = w + (int64_t)b * S;
  double acc = 0.0;
  for (int i = t; i < S; i += kDcemThreads) acc += (double)wb[i];
  const double W = dcem_block_sum(acc, red);
  const double hard_eps = mode == kDcemHard ? 1e-10 : 0.0;
  const double defect = (N - W) / N;

  // 256 columns at a time: their factors mu_j, gv_j, gmt_j once into LDS, then one wave per sample over the chunk's columns
  // (sample i belongs to wave i % 4 in every chunk: gw[i] has one writer and grows in a fixed order)
  for (int i = t; i < S; i += kDcemThreads) gw[i] = 0.0;
  for (int j0 = 0; j0 < n; j0 += kDcemThreads) {
    __syncthreads();   // (the chunk before has been read)
    if (j0 + t < n) {
      const int64_t cj = (int64_t)b * n + j0 + t;
      const double m = (double)mu[cj];
      const double gv = (double)grad_sigma[cj] / (2.0 * ((double)sigma[cj] - hard_eps));
      col_m[t] = m;
      col_gv[t] = gv;
      col_gmt[t] = (double)grad_mu[cj] - 2.0 * gv * m * defect;
    }
    __syncthreads();
    const int nc = n - j0 < kDcemThreads ? n - j0 : kDcemThreads;
    for (int i = wave; i < S; i += kDcemWaves) {
      const double wi = (double)wb[i];
      const int64_t row = ((int64_t)i * B + b) * n + j0;
      acc = 0.0;
      for (int c = lane; c < nc; c += 64) {
        const double gv = col_gv[c], gmt = col_gmt[c];
        const double x = (double)X[row + c], d = x - col_m[c];
        grad_X[row + c] = (T)(wi * (gmt + 2.0 * gv * d) / N);
        acc += (gmt * x + gv * d * d) / N;
      }
      acc = dcem_wave_sum(acc);
      if (lane == 0) gw[i] += acc;
    }
  }
  __syncthreads();

  const bool dead = mode == kDcemHard || (mode == kDcemLml && S <= n_elite);
  if (dead) {
    for (int i = t; i < S; i += kDcemThreads) grad_fX[(int64_t)i * B + b] = (T)0;
    return;
  }
  if (mode == kDcemLml) {
    double a0 = 0.0, a1 = 0.0;
    for (int i = t; i < S; i += kDcemThreads) {
      const double y = (double)wb[i];
      const double hinv = 1.0 / (1.0 / y + 1.0 / (1.0 - y));
      a0 += hinv * gw[i];
      a1 += hinv;
    }
    const double num = dcem_block_sum(a0, red), den = dcem_block_sum(a1, red);
    const double dnu = num / den;
    for (int i = t; i < S; i += kDcemThreads) {
      const double y = (double)wb[i];
      const double hinv = 1.0 / (1.0 / y + 1.0 / (1.0 - y));
      gw[i] = hinv * (gw[i] - dnu);
    }
  } else {
    double a0 = 0.0;
    for (int i = t; i < S; i += kDcemThreads) a0 += (double)wb[i] * gw[i];
    const double dot = dcem_block_sum(a0, red);
    for (int i = t; i < S; i += kDcemThreads) gw[i] = (double)wb[i] * (gw[i] - dot);
  }
  // x = -temp f:  dL/df = -temp dL/dx  (each thread touches only its own entries of gw: no barrier needed in between)
  for (int i = t; i < S; i += kDcemThreads) gw[i] = -(double)temp * gw[i];
  if (!normalize) {
    for (int i = t; i < S; i += kDcemThreads) grad_fX[(int64_t)i * B + b] = (T)gw[i];
    return;
  }
  // f_i = (u_i - m) c, c = 1 / (s + 1e-6), s the unbiased std:  dL/du_i = c (df_i - mean(df)) - c^2 sum_k df_k (u_k - m) (u_i - m) / ((S - 1) s)
  double mean, stdv;
  dcem_standardise<T>(fX, S, B, b, red, mean, stdv);
  double a0 = 0.0, a1 = 0.0;
  for (int i = t; i < S; i += kDcemThreads) {
    a0 += gw[i];
    a1 += gw[i] * ((double)fX[(int64_t)i * B + b] - mean);
  }
  const double sum_df = dcem_block_sum(a0, red), sum_dfu = dcem_block_sum(a1, red);
  const double s = stdv, cinv = 1.0 / (s + 1e-6);
  const double gs = -cinv * cinv * sum_dfu / ((double)(S - 1) * s);
  for (int i = t; i < S; i += kDcemThreads) {
    const double u = (double)fX[(int64_t)i * B + b] - mean;
    grad_fX[(int64_t)i * B + b] = (T)(cinv * (gw[i] - sum_df / (double)S) + gs * u);
  }
}

// what both exports check on the host before any launch
inline int dcem_check(const char* who, bool any_null, int32_t S, int32_t B, int32_t n, int32_t n_elite, int dtype) {
  if (any_null) return fail(who, ": null pointer");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (B < 1) return fail(who, ": empty batch");
  if (S < 1) return fail(who, ": S < 1");
  if (S > THX_DCEM_MAX_S) return fail(who, ": S > THX_DCEM_MAX_S (4096 samples: the scores of a problem stay in LDS)");
  if (n < 1) return fail(who, ": n < 1");
  if (n_elite < 1) return fail(who, ": n_elite < 1");
  return 0;
}

inline bool dcem_misaligned(int dtype, std::initializer_list<const void*> ps) {
  const uintptr_t el = dtype == THX_F32 ? 4 : 8;
  for (const void* p : ps)
    if (reinterpret_cast<uintptr_t>(p) % el) return true;
  return false;
}

}  // namespace thx

using namespace thx;

extern "C" int thx_dcem_update(const void* fX, const void* X, int32_t S, int32_t B, int32_t n, int32_t n_elite, double temp,
                               int normalize, double lml_eps, int32_t lml_n_iter, int32_t branch, void* mu, void* sigma, void* w,
                               void* nu, void* bracket, int32_t* flags, int dtype, void* stream) {
  const char* who = "thx_dcem_update";
  if (int rc = dcem_check(who, !fX || !X || !mu || !sigma || !w || !nu || !bracket || !flags, S, B, n, n_elite, dtype)) return rc;
  if (branch < 2) return fail(who, ": branch < 2");
  if (lml_n_iter < 0) return fail(who, ": lml_n_iter < 0");
  if (dcem_misaligned(dtype, {fX, X, mu, sigma, w, nu, bracket}) || reinterpret_cast<uintptr_t>(flags) % 4)
    return fail(who, ": pointer not aligned");
  const int mode = dcem_mode(temp, n_elite);
  const size_t el = dtype == THX_F32 ? 4 : 8;
  const size_t lds = (kDcemThreads + kDcemThreads / 2 + 2) * sizeof(double) + (size_t)S * el;
  const dim3 grid((unsigned)B), block(kDcemThreads);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(dcem_update_kernel<float>, grid, block, lds, as_stream(stream), (const float*)fX, (const float*)X,
                                  S, B, n, n_elite, (float)temp, normalize, (float)lml_eps, lml_n_iter, branch, mode, (float*)mu,
                                  (float*)sigma, (float*)w, (float*)nu, (float*)bracket, flags),
               hipLaunchKernelGGL(dcem_update_kernel<double>, grid, block, lds, as_stream(stream), (const double*)fX,
                                  (const double*)X, S, B, n, n_elite, temp, normalize, lml_eps, lml_n_iter, branch, mode,
                                  (double*)mu, (double*)sigma, (double*)w, (double*)nu, (double*)bracket, flags));
  return check_launch(who);
}

extern "C" int thx_dcem_update_vjp(const void* grad_mu, const void* grad_sigma, const void* X, const void* fX, const void* w,
                                   const void* mu, const void* sigma, int32_t S, int32_t B, int32_t n, int32_t n_elite, double temp,
                                   int normalize, void* grad_X, void* grad_fX, int dtype, void* stream) {
  const char* who = "thx_dcem_update_vjp";
  if (int rc = dcem_check(who, !grad_mu || !grad_sigma || !X || !fX || !w || !mu || !sigma || !grad_X || !grad_fX, S, B, n, n_elite,
                          dtype))
    return rc;
  if (dcem_misaligned(dtype, {grad_mu, grad_sigma, X, fX, w, mu, sigma, grad_X, grad_fX})) return fail(who, ": pointer not aligned");
  const int mode = dcem_mode(temp, n_elite);
  const size_t lds = (4 * kDcemThreads + (size_t)S) * sizeof(double);
  const dim3 grid((unsigned)B), block(kDcemThreads);
  THX_DISPATCH(dtype,
               hipLaunchKernelGGL(dcem_update_vjp_kernel<float>, grid, block, lds, as_stream(stream), (const float*)grad_mu,
                                  (const float*)grad_sigma, (const float*)X, (const float*)fX, (const float*)w, (const float*)mu,
                                  (const float*)sigma, S, B, n, n_elite, (float)temp, normalize, mode, (float*)grad_X,
                                  (float*)grad_fX),
               hipLaunchKernelGGL(dcem_update_vjp_kernel<double>, grid, block, lds, as_stream(stream), (const double*)grad_mu,
                                  (const double*)grad_sigma, (const double*)X, (const double*)fX, (const double*)w, (const double*)mu,
                                  (const double*)sigma, S, B, n, n_elite, temp, normalize, mode, (double*)grad_X, (double*)grad_fX));
  return check_launch(who);
}
