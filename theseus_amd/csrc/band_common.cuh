// What the banded-Cholesky sources share (band_kernels.hip: factor and single-vector solves; band_multi_kernels.hip: blocks of
// right-hand sides and the band of the inverse): the limits, the wave-level LDS fence, the lane broadcast and the size checks of the
// C entry points.  Lb (B, n, kd + 1): Lb[b, j, i] = L(j + i, j), column j one contiguous segment, zeros where j + i >= n.
#pragma once
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

// the wave's own LDS writes become visible to its reads.  LDS only ("local"): a fence over every address space also orders the
// column's store to Lb and the band columns in flight
__device__ __forceinline__ void band_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
}

inline int check_band_sizes(const char* who, int n, int kd, int B) {
  if (n <= 0 || B <= 0) return fail(who, ": need n > 0, B > 0");
  if (kd < 0 || kd >= n) return fail(who, ": need 0 <= kd < n");
  if (kd > BAND_MAX_KD) {
    const std::string msg = ": kd above the limit of " + std::to_string(BAND_MAX_KD) + " of the banded solver (one window row per lane)";
    return fail(who, msg.c_str());
  }
  return 0;
}

}  // namespace thx
