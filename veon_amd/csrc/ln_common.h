// What the LayerNorm / GELU training passes share (conv2d_train.hip on padded half images,
// linear_train.hip on token rows): GELU with its slope, the lane layout of a row of up to
// 1024 channels with its statistics, and the fixed-order second stage of the per-channel
// sums.  The lane and wave sums themselves (wave_sum, add_waves_in_order) are in
// lane_reduce.h.
#pragma once
#include "lane_reduce.h"
#include "mfma_common.h"

namespace {

// GELU (erf form) and its derivative from one rcp and one exp2:
//   h = erfc(|y| / sqrt 2) / 2,  Phi(y) = y > 0 ? 1 - h : h,  phi(y) = exp(-y^2 / 2) / sqrt(2 pi)
//   GELU(y) = y Phi(y) = max(y, 0) - |y| h,  GELU'(y) = Phi(y) + y phi(y)
// GELU takes h from the approximation of gelu_erf (mfma_common.h; |error| of Phi <= 8e-8),
// so that it equals the fused epilogue's.  GELU' takes it from a degree-7 polynomial in
// the same t (least squares in t weighted by t exp(-x^2), coefficients rounded to fp32 one
// at a time; |error| of h <= 5e-10 before rounding).  The error of the degree-4 fit has
// one sign over a stretch of y, so on a channel whose pixels all lie near y = -0.75, where
// GELU' crosses zero and sum |dx| is small, it added up over the rows of the sum of dx;
// what is left is the rounding of t and exp2 (about 1e-7, of either sign).  A caller that
// drops the slope pays nothing for it.
__device__ __forceinline__ void gelu_and_slope(float y, float* g, float* dg) {
  const float ay = fabsf(y);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752f, ay, 1.f));
  float p = fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
  p = fmaf(p, t, 0.5f * 1.421413741f);
  p = fmaf(p, t, 0.5f * -0.284496736f);
  p = fmaf(p, t, 0.5f * 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(ay * ay * -0.72134752044448170f);
  const float h = (p * t) * e;
  *g = fmaxf(y, 0.f) - ay * h;
  float q = fmaf(-3.500597551e-02f, t, 5.302065983e-02f);
  q = fmaf(q, t, 2.538232803e-01f);
  q = fmaf(q, t, -3.629937172e-01f);
  q = fmaf(q, t, 4.665356874e-01f);
  q = fmaf(q, t, -1.054019928e-01f);
  q = fmaf(q, t, 1.432103813e-01f);
  q = fmaf(q, t, 8.681167662e-02f);
  const float hs = (q * t) * e;
  *dg = fmaf(y * 0.39894228040143268f, e, y > 0.f ? 1.f - hs : hs);
}

// A lane holds N (1: C <= 512, 2: C <= 1024) 16-byte chunks of a padded row: channels
// 8 (lane + 64 h) + 0..7, h < N; has[h]: the row is wide enough for that chunk.
// One padded row of the wave as fp32, zeros where the lane has no chunk.
template <int N>
__device__ __forceinline__ void load_row(const bf16_t* p, int lane, const bool* has,
                                         float* v) {
#pragma unroll
  for (int h = 0; h < N; ++h) {
    bf16x8 c = {0, 0, 0, 0, 0, 0, 0, 0};
    if (has[h]) c = *reinterpret_cast<const bf16x8*>(p + (lane + 64 * h) * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[8 * h + k] = bf2f((bf16_t)c[k]);
  }
}

template <int N>
__device__ __forceinline__ void store_row(bf16_t* p, int lane, const bool* has,
                                          const float* v) {
#pragma unroll
  for (int h = 0; h < N; ++h) {
    if (!has[h]) continue;
    bf16x8 o8;
#pragma unroll
    for (int k = 0; k < 8; ++k) o8[k] = (short)f2bf(v[8 * h + k]);
    *reinterpret_cast<bf16x8*>(p + (lane + 64 * h) * 8) = o8;
  }
}

// mean and rstd of the lane-distributed row u (entries of absent chunks are ignored)
template <int N>
__device__ __forceinline__ void row_stats(const float* u, const bool* has, int C, float eps,
                                          float* mean, float* rstd) {
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 8 * N; ++k) sum += has[k >> 3] ? u[k] : 0.f;
  *mean = wave_sum(sum) / C;
  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < 8 * N; ++k) {
    const float a = has[k >> 3] ? u[k] - *mean : 0.f;
    sq = fmaf(a, a, sq);
  }
  *rstd = rsqrtf(wave_sum(sq) / C + eps);
}

constexpr int kLnBlocks = 1024;   // partial sums of stage one (upper bound)

// Stage two of every two-stage column sum: one wave per float4 of the sums (n4 of them,
// e.g. sums[3][C]).  Lane l adds the partials of workgroups
// l, l + 64, ... in that order, then the 64 lanes are added by a butterfly: a fixed
// order for a fixed number of workgroups, and log-depth instead of a serial walk.
__global__ __launch_bounds__(256) void k_ln_sums_final(const float4* __restrict__ part,
                                                       float4* __restrict__ sums, int n4,
                                                       int nblocks) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n4) return;   // wave-uniform
  float4 s = {0.f, 0.f, 0.f, 0.f};
  for (int b = lane; b < nblocks; b += 64) {
    const float4 v = part[(int64_t)b * n4 + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  s.x = wave_sum(s.x); s.y = wave_sum(s.y); s.z = wave_sum(s.z); s.w = wave_sum(s.w);
  if (lane == 0) sums[i] = s;
}

}  // namespace
