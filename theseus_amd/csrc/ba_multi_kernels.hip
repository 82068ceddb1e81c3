// Bundle adjustment, blocks of right-hand sides (include/theseus_hip.h: thx_ba_reduce_multi / thx_ba_backsub_multi): the point
// elimination and the back substitution of ba_kernels.hip for a (B, nrhs, n) block of vectors, one vector per row, so that the
// factor of the reduced camera system serves thx_chol_solve_multi / thx_chol_solve_multi_sparse on the camera columns of the block.
//
// With H = [[U, W], [W^T, V]] (cameras, then points), V^-1 = Hinv, S = U - W V^-1 W^T = L L^T and R R^T = V^-1 (R: the lower
// Cholesky factor of a point's packed Hinv, formed in registers), M = [[L, W R], [0, R^-T]] has M M^T = H, and
//   which = 0, x = H^-1 r:   reduce  xc = rc - W V^-1 rp,  xp = V^-1 rp;   solve xc = S^-1 xc;     backsub  xp -= V^-1 W^T xc
//   which = 2, y = M^-1 r:   reduce  yc = rc - W V^-1 rp,  yp = R^T rp;    solve yc = L^-1 yc
//   which = 1, x = M^-T z:                                                 solve xc = L^-T zc;     backsub  xp = R zp - V^-1 W^T xc
//
// Mapping: lane = problem, as everywhere on this path -- W (O, 18, B) and Hinv (Np, 6, B) are fp64 planar with
// the batch innermost, so a wave's load of one component is 512 contiguous bytes.  A workgroup owns one entity (a camera in the
// reduce pass, a point in the back substitution), 64 problems and a group of up to 32 vectors; it walks the entity's CSR list
// (cam_ptr / cam_obs, pt_ptr / pt_obs) in order, keeps the observation's block (times the point's inverse) in registers and
// applies it to every vector of the group: W and Hinv are read once per group of vectors.  The sums of all vectors of the
// group live in fp64 registers (96 per lane: 3 rows x 32 vectors; the 6 rows of a camera are split between the two waves of its
// workgroup).  The block of vectors has the problem as its SLOWEST index: a lane's own elements are bstride apart.  So the
// (64 problems x 3 or 6 columns x 8 vectors) patch an observation needs is staged through LDS: the threads walk it with the
// column fastest, then the vector, then the problem -- whole runs of the entity's columns per (problem, vector), 8 to 21
// lines per load instruction instead of 64 -- and each lane then reads its own problem's row of the patch (row stride 49:
// conflict free).  8 vectors at a time keep the patch at 12.25 KB (fp32) / 24.5 KB (fp64), so registers, not LDS, bound the
// occupancy.  No atomics: every output element has one owner and a fixed summation order -- the same input gives the same bits.
#include "common.cuh"

namespace thx {

constexpr int BM_G = 32;                 // vectors per group (accumulators in registers)
constexpr int BM_SV = 8;                 // vectors per staged patch
constexpr int BM_ROW = BM_SV * 6 + 1;    // LDS row of one problem: (vector, column), padded to an odd stride
constexpr int BM_LDS = 64 * BM_ROW;

// the planar fp64 workspaces of ba_kernels.hip: (entity, component, B)
template <int NC>
__device__ __forceinline__ int64_t bm_at(int64_t entity, int i, int b, int B) {
  return (entity * NC + i) * (int64_t)B + b;
}

// where a workgroup's patch of the block lives
template <typename T>
struct BmBlock {
  T* p;               // element (b, v, i) at b * bstride + v * ldv + i
  int64_t ldv, bstride;
  int b0, nb;         // problems b0 .. b0 + nb - 1 (nb <= 64)
};

// patch rows <- columns col0 .. col0 + NC - 1 of vectors v0 .. v0 + nv - 1 (nv <= BM_SV) of the workgroup's problems
template <typename T, int NC, int NT>
__device__ __forceinline__ void bm_stage_in(T* __restrict__ buf, const BmBlock<const T>& g, int v0, int nv, int64_t col0) {
  for (int f = threadIdx.x; f < 64 * BM_SV * NC; f += NT) {
    const int j = f % NC, r = f / NC, v = r % BM_SV, bl = r / BM_SV;
    if (v < nv && bl < g.nb) buf[bl * BM_ROW + v * 6 + j] = g.p[(int64_t)(g.b0 + bl) * g.bstride + (int64_t)(v0 + v) * g.ldv + col0 + j];
  }
}

template <typename T, int NC, int NT>
__device__ __forceinline__ void bm_stage_out(const T* __restrict__ buf, const BmBlock<T>& g, int v0, int nv, int64_t col0) {
  for (int f = threadIdx.x; f < 64 * BM_SV * NC; f += NT) {
    const int j = f % NC, r = f / NC, v = r % BM_SV, bl = r / BM_SV;
    if (v < nv && bl < g.nb) g.p[(int64_t)(g.b0 + bl) * g.bstride + (int64_t)(v0 + v) * g.ldv + col0 + j] = buf[bl * BM_ROW + v * 6 + j];
  }
}

// lower Cholesky factor R (r00 r10 r11 r20 r21 r22) of the packed symmetric 3 x 3 h = (a b c d e f)
__device__ __forceinline__ void bm_chol3(const double* h, double* R) {
  R[0] = sqrt(h[0]);
  R[1] = h[1] / R[0];
  R[3] = h[2] / R[0];
  R[2] = sqrt(h[3] - R[1] * R[1]);
  R[4] = (h[4] - R[3] * R[1]) / R[2];
  R[5] = sqrt(h[5] - R[3] * R[3] - R[4] * R[4]);
}

// ---- reduce, cameras: xc = rc - sum_o W_o V^-1 rp(o) over the camera's observations.  Two waves: wave h owns rows 3h .. 3h + 2
//      of the camera (its half of W, times the point's inverse, in registers); both stage and read one patch.
template <typename T>
__global__ void __launch_bounds__(128)
ba_reduce_cam_multi_kernel(thx_ba_structure s, int B, const double* __restrict__ W, const double* __restrict__ Hinv,
                           const T* rhs, T* x, int nrhs, int64_t ldv, int64_t bstride) {
  __shared__ T buf[BM_LDS];
  const int c = blockIdx.x, b0 = blockIdx.y * 64, vg = blockIdx.z * BM_G, ng = min(BM_G, nrhs - vg);
  const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
  const int b = min(b0 + lane, B - 1);   // (lanes past the batch compute on the last problem; their rows are never staged out)
  const BmBlock<const T> in{rhs, ldv, bstride, b0, min(64, B - b0)};
  const BmBlock<T> out{x, ldv, bstride, b0, min(64, B - b0)};
  const int64_t pcol = 6 * (int64_t)s.num_cams;
  const T* row = buf + lane * BM_ROW;
  double acc[BM_G][3];
#pragma unroll
  for (int v = 0; v < BM_G; ++v) acc[v][0] = acc[v][1] = acc[v][2] = 0.0;
  for (int k = s.cam_ptr[c]; k < s.cam_ptr[c + 1]; ++k) {
    const int o = s.cam_obs[k], p = s.obs_pt[o];
    double w[9], hh[6], M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = W[bm_at<18>(o, 9 * h + i, b, B)];
#pragma unroll
    for (int i = 0; i < 6; ++i) hh[i] = Hinv[bm_at<6>(p, i, b, B)];
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // M = W_half * V^-1
      M[3 * i] = w[3 * i] * hh[0] + w[3 * i + 1] * hh[1] + w[3 * i + 2] * hh[2];
      M[3 * i + 1] = w[3 * i] * hh[1] + w[3 * i + 1] * hh[3] + w[3 * i + 2] * hh[4];
      M[3 * i + 2] = w[3 * i] * hh[2] + w[3 * i + 1] * hh[4] + w[3 * i + 2] * hh[5];
    }
#pragma unroll
    for (int vs = 0; vs < BM_G / BM_SV; ++vs) {
      if (vs * BM_SV < ng) {   // (workgroup uniform)
        __syncthreads();
        bm_stage_in<T, 3, 128>(buf, in, vg + vs * BM_SV, min(BM_SV, ng - vs * BM_SV), pcol + 3 * (int64_t)p);
        __syncthreads();
#pragma unroll
        for (int vv = 0; vv < BM_SV; ++vv) {
          if (vs * BM_SV + vv < ng) {
            const double r0 = (double)row[vv * 6], r1 = (double)row[vv * 6 + 1], r2 = (double)row[vv * 6 + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[vs * BM_SV + vv][i] += M[3 * i] * r0 + M[3 * i + 1] * r1 + M[3 * i + 2] * r2;
          }
        }
      }
    }
  }
#pragma unroll
  for (int vs = 0; vs < BM_G / BM_SV; ++vs) {
    if (vs * BM_SV < ng) {
      const int nv = min(BM_SV, ng - vs * BM_SV);
      __syncthreads();
      bm_stage_in<T, 6, 128>(buf, in, vg + vs * BM_SV, nv, 6 * (int64_t)c);
      __syncthreads();
#pragma unroll
      for (int vv = 0; vv < BM_SV; ++vv) {
        if (vs * BM_SV + vv < ng) {
          T* e = buf + lane * BM_ROW + vv * 6 + 3 * h;   // (this lane's own three elements)
#pragma unroll
          for (int i = 0; i < 3; ++i) e[i] = (T)((double)e[i] - acc[vs * BM_SV + vv][i]);
        }
      }
      __syncthreads();
      bm_stage_out<T, 6, 128>(buf, out, vg + vs * BM_SV, nv, 6 * (int64_t)c);
    }
  }
}

// ---- reduce, points: xp = V^-1 rp (which = 0) or R^T rp (which = 2) ----
template <typename T>
__global__ void __launch_bounds__(64)
ba_reduce_pt_multi_kernel(thx_ba_structure s, int B, const double* __restrict__ Hinv, const T* rhs, T* x, int nrhs,
                          int64_t ldv, int64_t bstride, int which) {
  __shared__ T buf[BM_LDS];
  const int p = blockIdx.x, b0 = blockIdx.y * 64, vg = blockIdx.z * BM_G, ng = min(BM_G, nrhs - vg);
  const int lane = threadIdx.x, b = min(b0 + lane, B - 1);
  const BmBlock<const T> in{rhs, ldv, bstride, b0, min(64, B - b0)};
  const BmBlock<T> out{x, ldv, bstride, b0, min(64, B - b0)};
  const int64_t col = 6 * (int64_t)s.num_cams + 3 * (int64_t)p;
  double hh[6], R[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) hh[i] = Hinv[bm_at<6>(p, i, b, B)];
  bm_chol3(hh, R);
  for (int v0 = 0; v0 < ng; v0 += BM_SV) {
    const int nv = min(BM_SV, ng - v0);
    __syncthreads();
    bm_stage_in<T, 3, 64>(buf, in, vg + v0, nv, col);
    __syncthreads();
    for (int vv = 0; vv < nv; ++vv) {
      T* e = buf + lane * BM_ROW + vv * 6;
      const double r0 = (double)e[0], r1 = (double)e[1], r2 = (double)e[2];
      if (which == 0) {
        e[0] = (T)(hh[0] * r0 + hh[1] * r1 + hh[2] * r2);
        e[1] = (T)(hh[1] * r0 + hh[3] * r1 + hh[4] * r2);
        e[2] = (T)(hh[2] * r0 + hh[4] * r1 + hh[5] * r2);
      } else {
        e[0] = (T)(R[0] * r0 + R[1] * r1 + R[3] * r2);
        e[1] = (T)(R[2] * r1 + R[4] * r2);
        e[2] = (T)(R[5] * r2);
      }
    }
    __syncthreads();
    bm_stage_out<T, 3, 64>(buf, out, vg + v0, nv, col);
  }
}

// ---- back substitution: xp = own - V^-1 sum_o W_o^T xc(o) over the point's observations; own = xp as the reduce pass left it
//      (which = 0) or R zp (which = 1).  In place on x: the camera columns are only read, a point's columns have one owner.
template <typename T>
__global__ void __launch_bounds__(64)
ba_backsub_multi_kernel(thx_ba_structure s, int B, const double* __restrict__ W, const double* __restrict__ Hinv, T* x, int nrhs,
                        int64_t ldv, int64_t bstride, int which) {
  __shared__ T buf[BM_LDS];
  const int p = blockIdx.x, b0 = blockIdx.y * 64, vg = blockIdx.z * BM_G, ng = min(BM_G, nrhs - vg);
  const int lane = threadIdx.x, b = min(b0 + lane, B - 1);
  const BmBlock<const T> in{x, ldv, bstride, b0, min(64, B - b0)};
  const BmBlock<T> out{x, ldv, bstride, b0, min(64, B - b0)};
  const int64_t col = 6 * (int64_t)s.num_cams + 3 * (int64_t)p;
  const T* row = buf + lane * BM_ROW;
  double acc[BM_G][3];
#pragma unroll
  for (int v = 0; v < BM_G; ++v) acc[v][0] = acc[v][1] = acc[v][2] = 0.0;
  for (int k = s.pt_ptr[p]; k < s.pt_ptr[p + 1]; ++k) {
    const int o = s.pt_obs[k], c = s.obs_cam[o];
    double w[18];
#pragma unroll
    for (int i = 0; i < 18; ++i) w[i] = W[bm_at<18>(o, i, b, B)];
#pragma unroll
    for (int vs = 0; vs < BM_G / BM_SV; ++vs) {
      if (vs * BM_SV < ng) {
        __syncthreads();
        bm_stage_in<T, 6, 64>(buf, in, vg + vs * BM_SV, min(BM_SV, ng - vs * BM_SV), 6 * (int64_t)c);
        __syncthreads();
#pragma unroll
        for (int vv = 0; vv < BM_SV; ++vv) {
          if (vs * BM_SV + vv < ng) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const double di = (double)row[vv * 6 + i];
#pragma unroll
              for (int j = 0; j < 3; ++j) acc[vs * BM_SV + vv][j] += w[3 * i + j] * di;
            }
          }
        }
      }
    }
  }
  double hh[6], R[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) hh[i] = Hinv[bm_at<6>(p, i, b, B)];
  bm_chol3(hh, R);
#pragma unroll
  for (int vs = 0; vs < BM_G / BM_SV; ++vs) {
    if (vs * BM_SV < ng) {
      const int nv = min(BM_SV, ng - vs * BM_SV);
      __syncthreads();
      bm_stage_in<T, 3, 64>(buf, in, vg + vs * BM_SV, nv, col);
      __syncthreads();
#pragma unroll
      for (int vv = 0; vv < BM_SV; ++vv) {
        if (vs * BM_SV + vv < ng) {
          T* e = buf + lane * BM_ROW + vv * 6;
          const double a[3] = {acc[vs * BM_SV + vv][0], acc[vs * BM_SV + vv][1], acc[vs * BM_SV + vv][2]};
          double o0 = (double)e[0], o1 = (double)e[1], o2 = (double)e[2];
          if (which == 1) {   // R zp
            const double z0 = o0, z1 = o1, z2 = o2;
            o0 = R[0] * z0;
            o1 = R[1] * z0 + R[2] * z1;
            o2 = R[3] * z0 + R[4] * z1 + R[5] * z2;
          }
          e[0] = (T)(o0 - (hh[0] * a[0] + hh[1] * a[1] + hh[2] * a[2]));
          e[1] = (T)(o1 - (hh[1] * a[0] + hh[3] * a[1] + hh[4] * a[2]));
          e[2] = (T)(o2 - (hh[2] * a[0] + hh[4] * a[1] + hh[5] * a[2]));
        }
      }
      __syncthreads();
      bm_stage_out<T, 3, 64>(buf, out, vg + vs * BM_SV, nv, col);
    }
  }
}

static int check_ba_multi(const char* who, const thx_ba_structure* s, int32_t B, const void* W, const void* Hinv, const void* rhs,
                          const void* x, int32_t nrhs, int64_t ldv, int64_t bstride, int which, int dtype) {
  if (!s || !Hinv || !rhs || !x || (s->num_obs > 0 && !W)) return fail(who, ": null pointer");
  if (s->num_cams <= 0 || s->num_points <= 0 || B <= 0) return fail(who, ": need cameras, points and B>0");
  if (nrhs < 1) return fail(who, ": nrhs < 1");
  if (ldv < 6 * (int64_t)s->num_cams + 3 * (int64_t)s->num_points) return fail(who, ": ldv < n");
  if (bstride / nrhs < ldv) return fail(who, ": bstride < nrhs * ldv");   // (no product: nrhs * ldv may not fit)
  if (which < 0 || which > 2) return fail(who, ": which = 0 (H^-1), 1 (M^-T), 2 (M^-1)");
  if (dtype != THX_F32 && dtype != THX_F64) return fail(who, ": bad dtype");
  if (((int64_t)B + 63) / 64 > 65535 || ((int64_t)nrhs + BM_G - 1) / BM_G > 65535)
    return fail(who, ": ceil(B / 64) or ceil(nrhs / 32) exceeds the grid limit");
  return 0;
}

template <typename T>
static void reduce_multi_launch(const thx_ba_structure* s, int B, const void* W, const void* Hinv, const void* rhs, void* x, int nrhs,
                                int64_t ldv, int64_t bstride, int which, hipStream_t st) {
  const unsigned chunks = (unsigned)((B + 63) / 64), groups = (unsigned)((nrhs + BM_G - 1) / BM_G);
  // cameras first: they read the point columns of rhs, which the point pass overwrites when x is rhs
  ba_reduce_cam_multi_kernel<T><<<dim3((unsigned)s->num_cams, chunks, groups), dim3(128), 0, st>>>(
      *s, B, static_cast<const double*>(W), static_cast<const double*>(Hinv), static_cast<const T*>(rhs), static_cast<T*>(x), nrhs,
      ldv, bstride);
  ba_reduce_pt_multi_kernel<T><<<dim3((unsigned)s->num_points, chunks, groups), dim3(64), 0, st>>>(
      *s, B, static_cast<const double*>(Hinv), static_cast<const T*>(rhs), static_cast<T*>(x), nrhs, ldv, bstride, which);
}

template <typename T>
static void backsub_multi_launch(const thx_ba_structure* s, int B, const void* W, const void* Hinv, void* x, int nrhs, int64_t ldv,
                                 int64_t bstride, int which, hipStream_t st) {
  const unsigned chunks = (unsigned)((B + 63) / 64), groups = (unsigned)((nrhs + BM_G - 1) / BM_G);
  ba_backsub_multi_kernel<T><<<dim3((unsigned)s->num_points, chunks, groups), dim3(64), 0, st>>>(
      *s, B, static_cast<const double*>(W), static_cast<const double*>(Hinv), static_cast<T*>(x), nrhs, ldv, bstride, which);
}

}  // namespace thx

using namespace thx;

extern "C" {

int thx_ba_reduce_multi(const thx_ba_structure* s, int32_t B, const void* W, const void* Hinv, const void* rhs, void* x, int32_t nrhs,
                        int64_t ldv, int64_t bstride, int which, int dtype, void* stream) {
  const char* who = "thx_ba_reduce_multi";
  if (int r = check_ba_multi(who, s, B, W, Hinv, rhs, x, nrhs, ldv, bstride, which, dtype)) return r;
  if (which == 1) return 0;   // (M^-T has no reduce pass)
  THX_DISPATCH(dtype, reduce_multi_launch<float>(s, B, W, Hinv, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)),
               reduce_multi_launch<double>(s, B, W, Hinv, rhs, x, nrhs, ldv, bstride, which, as_stream(stream)));
  return check_launch(who);
}

int thx_ba_backsub_multi(const thx_ba_structure* s, int32_t B, const void* W, const void* Hinv, void* x, int32_t nrhs, int64_t ldv,
                         int64_t bstride, int which, int dtype, void* stream) {
  const char* who = "thx_ba_backsub_multi";
  if (int r = check_ba_multi(who, s, B, W, Hinv, x, x, nrhs, ldv, bstride, which, dtype)) return r;
  if (which == 2) return 0;   // (M^-1 leaves the points as the reduce pass wrote them)
  THX_DISPATCH(dtype, backsub_multi_launch<float>(s, B, W, Hinv, x, nrhs, ldv, bstride, which, as_stream(stream)),
               backsub_multi_launch<double>(s, B, W, Hinv, x, nrhs, ldv, bstride, which, as_stream(stream)));
  return check_launch(who);
}

}  // extern "C"
