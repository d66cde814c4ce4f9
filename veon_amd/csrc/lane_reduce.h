// Reductions over the lanes of a wave and the waves of a workgroup (device only).  The
// ORDER of every sum here is part of its contract: fp32 / fp64 addition does not
// associate, and the exact seam tests pin these orders bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Xor butterfly over the 64 lanes of a wave, partners at distance 32, 16, ..., 1 in that
// order: every lane gets the same bits.  T: float or double.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
  for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

// Sum over the 32 lanes of a half wave; every lane gets the same bits (each step adds
// a lane's value to its partner's in both lanes, and fp32 addition commutes).  DPP
// inside the 16-lane rows (quad xor 1, quad xor 2, half-row mirror, row mirror), then
// v_permlane16_swap pairs rows 0/1 and 2/3 (asm with its wait states, as
// max_over_rows of attention_kernel.h).
__device__ __forceinline__ float half_wave_sum(float x) {
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                     0, __builtin_bit_cast(int, x), 0xB1, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                     0, __builtin_bit_cast(int, x), 0x4E, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                     0, __builtin_bit_cast(int, x), 0x141, 0xf, 0xf, false));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
                                     0, __builtin_bit_cast(int, x), 0x140, 0xf, 0xf, false));
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return a + b;
}

// Sums K values over the workgroup of W waves in a fixed order: the butterfly inside each
// wave, lane 0 of each wave to red[k][wave] (red has at least K rows), then every thread
// adds the W waves in index order.  Needs a barrier before red[] is written again.
template <int K, int W, typename T>
__device__ __forceinline__ void block_sum(T (&vals)[K], T (*red)[W]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) vals[k] = wave_sum(vals[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][wave] = vals[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) vals[k] = T(0);
  for (int i = 0; i < W; ++i) {
#pragma unroll
    for (int k = 0; k < K; ++k) vals[k] += red[k][i];
  }
}

// Per-lane sums of the four waves of a 256-thread workgroup, in two steps.  park_waves
// (all threads): waves 1..3 leave their acc[k] at red[wave - 1][k * 64 + lane], then a
// barrier.  add_waves_in_order (wave 0, by value and inside the caller's own
// `if (wave == 0 ...)`: a helper that took the array and branched itself compiled to a
// second branch and other LDS reads): wave 0's own w0 plus entry i of the parked ones,
// associated ((w0 + w1) + w2) + w3.  Needs a barrier before red[] is written again.
template <int K, typename T>
__device__ __forceinline__ void park_waves(const T* acc, T (&red)[3][K * 64], int lane,
                                           int wave) {
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave - 1][k * 64 + lane] = acc[k];
  }
  __syncthreads();
}

__device__ __forceinline__ float sum_in_order(float w0, float w1, float w2, float w3) {
  return ((w0 + w1) + w2) + w3;
}

template <int N>
__device__ __forceinline__ float add_waves_in_order(float w0, const float (&red)[3][N],
                                                    int i) {
  return sum_in_order(w0, red[0][i], red[1][i], red[2][i]);
}

template <int N>
__device__ __forceinline__ float4 add_waves_in_order(float4 w0, const float4 (&red)[3][N],
                                                     int i) {
  const float4 a = red[0][i], b = red[1][i], c = red[2][i];
  return float4{sum_in_order(w0.x, a.x, b.x, c.x), sum_in_order(w0.y, a.y, b.y, c.y),
                sum_in_order(w0.z, a.z, b.z, c.z), sum_in_order(w0.w, a.w, b.w, c.w)};
}

}  // namespace
