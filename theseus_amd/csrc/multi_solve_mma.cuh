// What the multi-right-hand-side triangular solves share (multi_solve_kernels.hip on the dense frame, sparse_multi_kernels.hip
// on the tile pattern): the chunk geometry, one wave's 32 x 32 (x 32) product on the matrix cores and the 16-byte load vectors.
#pragma once

namespace thx {

constexpr int MS_TILE = 128;             // block row (THX_TILE)
constexpr int MS_KC = 32;                // K extent of a chunk
constexpr int MS_G = 32;                 // right-hand sides per workgroup
constexpr int MS_LSA = MS_KC + 1;        // chunk of L as it is multiplied forward: sA[r * MS_LSA + k], r < 128, k < 32
constexpr int MS_LST = MS_TILE + 4;      // chunk of L read as rows, used transposed: sA[k * MS_LST + r]
constexpr int MS_LSB = MS_G + 1;         // chunk of X: sB[k * MS_LSB + s]
constexpr int MS_SA = MS_TILE * MS_LSA;  // (= 4224 = MS_KC * MS_LST)
static_assert(MS_SA == MS_KC * MS_LST, "one buffer serves both layouts");

typedef float ms_f32x16 __attribute__((ext_vector_type(16)));
typedef double ms_f64x4 __attribute__((ext_vector_type(4)));

// One wave's 32 x 32 (x 32) product on the matrix cores, D += A B.  A(i, k) = sA[i * AIS + k * AKS], B(k, j) = sB[k * MS_LSB + j].
// A lane holds 16 elements of D; element e sits at (row(e, lane), col(e, lane)).
template <typename T>
struct MsMma;

template <>
struct MsMma<float> {   // v_mfma_f32_32x32x2_f32: lane (i = l & 31, k = l >> 5) of A, (k, j = l & 31) of B
  using Frag = ms_f32x16;
  static __device__ __forceinline__ int row(int e, int l) { return 8 * (e >> 2) + 4 * (l >> 5) + (e & 3); }
  static __device__ __forceinline__ int col(int, int l) { return l & 31; }
  static __device__ __forceinline__ float get(const Frag& d, int e) { return d[e]; }
  static __device__ __forceinline__ void set(Frag& d, int e, float x) { d[e] = x; }
  template <int AIS, int AKS>
  static __device__ __forceinline__ void mac(Frag& d, const float* sA, const float* sB, int l) {
    const int i = l & 31, g = l >> 5;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 2 * kk + g;
      d = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[i * AIS + k * AKS], sB[k * MS_LSB + i], d, 0, 0, 0);
    }
  }
};

template <>
struct MsMma<double> {   // v_mfma_f64_16x16x4_f64, two 16-column halves of two 16-row halves: lane (i = l & 15, k = l >> 4)
  struct Frag {
    ms_f64x4 v[4];   // block (ih, jh) = v[2 ih + jh]
  };
  static __device__ __forceinline__ int row(int e, int l) { return 16 * (e >> 3) + 4 * (e & 3) + (l >> 4); }
  static __device__ __forceinline__ int col(int e, int l) { return 16 * ((e >> 2) & 1) + (l & 15); }
  static __device__ __forceinline__ double get(const Frag& d, int e) { return d.v[e >> 2][e & 3]; }
  static __device__ __forceinline__ void set(Frag& d, int e, double x) { d.v[e >> 2][e & 3] = x; }
  template <int AIS, int AKS>
  static __device__ __forceinline__ void mac(Frag& d, const double* sA, const double* sB, int l) {
    const int i = l & 15, g = l >> 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int k = 4 * kk + g;
      const double a0 = sA[i * AIS + k * AKS], a1 = sA[(16 + i) * AIS + k * AKS];
      const double b0 = sB[k * MS_LSB + i], b1 = sB[k * MS_LSB + 16 + i];
      d.v[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, d.v[0], 0, 0, 0);
      d.v[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, d.v[1], 0, 0, 0);
      d.v[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, d.v[2], 0, 0, 0);
      d.v[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, d.v[3], 0, 0, 0);
    }
  }
};

template <typename T>
struct MsVec;
template <>
struct MsVec<float> {
  using V = float4;
  static constexpr int NV = 4;
  static __device__ __forceinline__ float at(const V& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
  static __device__ __forceinline__ V zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <>
struct MsVec<double> {
  using V = double2;
  static constexpr int NV = 2;
  static __device__ __forceinline__ double at(const V& v, int e) { return e == 0 ? v.x : v.y; }
  static __device__ __forceinline__ V zero() { return make_double2(0.0, 0.0); }
};

}  // namespace thx
