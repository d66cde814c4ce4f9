// Training of the token-wise layers of the HSA network (FeedForward heads and token
// LayerNorms, highres_side_adaptor.py:55-66, 108-193) on plain rows:
//     xn = LN(x)                 x fp32 tokens [T][d], xn half (veon_vit_layernorm)
//     y1 = xn W1^T + b1          half (veon_vit_gemm)
//     h  = GELU(y1)              half                          veon_gelu_bf16
//     y  = h W2^T + b2           half (veon_vit_gemm)
// and backwards, given dy (half):
//     db2 = sum_rows dy                                         veon_rows_colsum_bf16
//     dW2[n][k] = sum_rows dy[row][n] h[row][k]                 veon_linear_wgrad_bf16
//     dh  = dy W2                (veon_vit_gemm on the transposed weight)
//     dy1 = dh GELU'(y1)                                        veon_gelu_bwd_bf16
//     db1, dW1 from (dy1, xn), dxn = dy1 W1
//     dx, dgamma, dbeta = LN'(dxn; x)                           veon_layernorm_f32_bwd
//
// The weight gradient is the kernel of wgrad_kernel.h (shared with conv3d_train.hip and
// conv2d_train.hip) as its one-tap case: no row offset, one workgroup per (N, K) tile and
// split of the rows.  Token matrices have no guard rows: the kernel's resources end at
// row M and the tail of a partial last slab is zeroed in LDS.
//
// The LayerNorm backward keeps k_image_layernorm_bwd's structure on fp32 rows: one wave
// per row, statistics recomputed from x, per-lane running sums, two stages in a fixed
// order.
#include "mfma_common.h"
#include "ln_common.h"
#include "wgrad_kernel.h"

namespace {

constexpr int kColBlocks = 512;   // row blocks of the column sum's stage one (upper bound)

// Stage one of sums[N] = sum over the rows of dy [M][N] (half).  Workgroup (bx, by): the
// 64 16-byte chunks bx of rows [by rows_per_block, ...); wave w walks rows w, w + 4, ...
// with 8 running fp32 sums per lane, the four waves are added in wave order and
// part[by][N] is written.
__global__ __launch_bounds__(256) void k_rows_colsum(const bf16_t* __restrict__ dy,
                                                     float* __restrict__ part, int M, int N,
                                                     int rows_per_block) {
  __shared__ float red[3][8 * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = blockIdx.x * 64 + lane;
  const bool has = chunk < N / 8;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (has)
    for (int m = r0 + wave; m < r1; m += 4) {
      const bf16x8 c = *reinterpret_cast<const bf16x8*>(dy + (int64_t)m * N + chunk * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += bf2f((bf16_t)c[k]);
    }
  park_waves<8>(acc, red, lane, wave);
  if (wave == 0 && has) {
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = add_waves_in_order(acc[k], red, k * 64 + lane);
    float* q = part + (int64_t)blockIdx.y * N + chunk * 8;
    *reinterpret_cast<float4*>(q) = float4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<float4*>(q + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
  }
}

// h = GELU(y), or dy = dh GELU'(y): one 16-byte chunk per thread, fp32 from the stored
// half value, both from gelu_and_slope (one rcp, one exp2).  QUICK: CLIP's
// QuickGELU y sigma(1.702 y) and its slope sigma + 1.702 y sigma (1 - sigma).
template <bool BWD, bool QUICK = false>
__global__ __launch_bounds__(256) void k_gelu(const bf16_t* __restrict__ y,
                                              const bf16_t* __restrict__ dh,
                                              bf16_t* __restrict__ out, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const bf16x8 c = reinterpret_cast<const bf16x8*>(y)[i];
  bf16x8 d = {0, 0, 0, 0, 0, 0, 0, 0}, o;
  if (BWD) d = reinterpret_cast<const bf16x8*>(dh)[i];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float g, slope;
    if (QUICK) {
      const float yv = bf2f((bf16_t)c[k]);
      const float sg = 1.f / (1.f + __expf(-1.702f * yv));
      g = yv * sg;
      // where sigma has saturated the second term is 0; evaluated as written it is
      // inf * 0 for the largest bf16 arguments (1.702 |y| overflows fp32)
      slope = sg * (1.f - sg) == 0.f ? sg : sg + 1.702f * yv * sg * (1.f - sg);
    } else {
      gelu_and_slope(bf2f((bf16_t)c[k]), &g, &slope);
    }
    o[k] = (short)f2bf(BWD ? bf2f((bf16_t)d[k]) * slope : g);
  }
  reinterpret_cast<bf16x8*>(out)[i] = o;
}

// One fp32 row of the wave: channels 8 (lane + 64 h) + 0..7, zeros where the lane has no
// chunk (the layout of load_row).
template <int N>
__device__ __forceinline__ void load_row_f32(const float* p, int lane, const bool* has,
                                             float* v) {
#pragma unroll
  for (int h = 0; h < N; ++h) {
    float4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (has[h]) {
      lo = *reinterpret_cast<const float4*>(p + (lane + 64 * h) * 8);
      hi = *reinterpret_cast<const float4*>(p + (lane + 64 * h) * 8 + 4);
    }
    v[8 * h + 0] = lo.x; v[8 * h + 1] = lo.y; v[8 * h + 2] = lo.z; v[8 * h + 3] = lo.w;
    v[8 * h + 4] = hi.x; v[8 * h + 5] = hi.y; v[8 * h + 6] = hi.z; v[8 * h + 7] = hi.w;
  }
}

// LayerNorm backward on fp32 token rows, stage one of the sums.  Workgroup b walks rows
// [b rows_per_block, (b + 1) rows_per_block), wave w of it rows w, w + 4, ...:
//   xhat = (x - mean) rstd,  a = dout gamma,  dx = rstd (a - mean(a) - xhat mean(a xhat))
// written as fp32, and every lane keeps the running sums of its 8 N channels: dout xhat,
// dout.  At the end the four waves are added in wave order and part[b][2][d] is written.
template <bool DOUT_HALF, int N>
__global__ __launch_bounds__(256) void k_layernorm_f32_bwd(
    const void* __restrict__ dout, const float* __restrict__ x,
    const float* __restrict__ gamma, float* __restrict__ dx, float* __restrict__ part,
    int T, int C, float eps, int rows_per_block) {
  constexpr int E = 8 * N;                 // channels per lane
  __shared__ float red[3][2 * E * 64];     // waves 1..3: [sum * E + k][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = C / 8;
  const bool has[2] = {lane < nchunk, N == 2 && lane + 64 < nchunk};
  float gm[E], acc[2 * E];
#pragma unroll
  for (int k = 0; k < E; ++k)
    gm[k] = has[k >> 3] ? gamma[(lane + 64 * (k >> 3)) * 8 + (k & 7)] : 0.f;
#pragma unroll
  for (int k = 0; k < 2 * E; ++k) acc[k] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < T ? r0 + rows_per_block : T;
  for (int64_t m = r0 + wave; m < r1; m += 4) {
    float u[E], d[E];
    load_row_f32<N>(x + m * C, lane, has, u);
    if (DOUT_HALF)
      load_row<N>(static_cast<const bf16_t*>(dout) + m * C, lane, has, d);
    else
      load_row_f32<N>(static_cast<const float*>(dout) + m * C, lane, has, d);
    float mean, rstd;
    row_stats<N>(u, has, C, eps, &mean, &rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      // absent chunks: d = gm = 0, so they add nothing to any sum
      u[k] = (u[k] - mean) * rstd;          // xhat
      const float a = d[k] * gm[k];
      s1 += a;
      s2 = fmaf(a, u[k], s2);
    }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      acc[k] = fmaf(d[k], u[k], acc[k]);
      acc[E + k] += d[k];
      d[k] = rstd * (d[k] * gm[k] - s1 - u[k] * s2);
    }
#pragma unroll
    for (int h = 0; h < N; ++h) {
      if (!has[h]) continue;
      float* q = dx + m * C + (lane + 64 * h) * 8;
      const float* a = d + 8 * h;
      *reinterpret_cast<float4*>(q) = float4{a[0], a[1], a[2], a[3]};
      *reinterpret_cast<float4*>(q + 4) = float4{a[4], a[5], a[6], a[7]};
    }
  }
  park_waves<2 * E>(acc, red, lane, wave);
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < 2 * E; ++k) acc[k] = add_waves_in_order(acc[k], red, k * 64 + lane);
    float* o = part + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int h = 0; h < N; ++h) {
        if (!has[h]) continue;
        float* q = o + s * C + (lane + 64 * h) * 8;
        const float* a = acc + E * s + 8 * h;
        *reinterpret_cast<float4*>(q) = float4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<float4*>(q + 4) = float4{a[4], a[5], a[6], a[7]};
      }
  }
}

bool ln_width_ok(int d) { return d > 0 && d % 64 == 0 && d <= 1024; }

}  // namespace

extern "C" {

int64_t veon_linear_wgrad_workspace_bytes(int M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return -1;
  return wgrad_workspace_bytes<0>(M, 0, K, N);
}

int veon_linear_wgrad_bf16(const void* dy, const void* x, float* dw, void* workspace,
                           int64_t workspace_bytes, int M, int K, int N, void* stream) {
  if (M <= 0 || K <= 0 || N <= 0) return VEON_ERR_BAD_ARG;
  return wgrad_run<0>(dy, x, dw, workspace, workspace_bytes, M, 0, 0, 0, K, N, stream);
}

int64_t veon_rows_colsum_workspace_bytes(int N) {
  if (N <= 0 || N % 8 != 0) return -1;
  return (int64_t)kColBlocks * N * (int64_t)sizeof(float);
}

int veon_rows_colsum_bf16(const void* dy, float* sums, void* workspace,
                          int64_t workspace_bytes, int M, int N, void* stream) {
  if (M <= 0 || N <= 0 || N % 8 != 0 || !dy || !sums || !workspace || !al16(dy) ||
      !al16(sums) || !al16(workspace))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_rows_colsum_workspace_bytes(N)) return VEON_ERR_WORKSPACE;
  // at least four rounds of rows per workgroup, at most kColBlocks row blocks
  int rows = (M + kColBlocks - 1) / kColBlocks;
  if (rows < 16) rows = 16;
  const int nblocks = (M + rows - 1) / rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_rows_colsum, dim3((unsigned)((N / 8 + 63) / 64), (unsigned)nblocks),
                     dim3(256), 0, s, static_cast<const bf16_t*>(dy), part, M, N, rows);
  const int n4 = N / 4;
  hipLaunchKernelGGL(k_ln_sums_final, dim3((n4 + 3) / 4), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(part), reinterpret_cast<float4*>(sums),
                     n4, nblocks);
  return launch_status();
}

int veon_gelu_bf16(const void* y, void* h, int64_t n, void* stream) {
  if (n <= 0 || n % 8 != 0 || n / 8 > 0x7fffffffLL * 256 || !y || !h || !al16(y) || !al16(h))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL((k_gelu<false>), dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(y),
                     static_cast<const bf16_t*>(nullptr), static_cast<bf16_t*>(h), n / 8);
  return launch_status();
}

int veon_gelu_bwd_bf16(const void* dh, const void* y, void* dy, int64_t n, void* stream) {
  if (n <= 0 || n % 8 != 0 || n / 8 > 0x7fffffffLL * 256 || !dh || !y || !dy || !al16(dh) ||
      !al16(y) || !al16(dy))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL((k_gelu<true>), dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(y),
                     static_cast<const bf16_t*>(dh), static_cast<bf16_t*>(dy), n / 8);
  return launch_status();
}

int veon_quickgelu_bf16(const void* y, void* h, int64_t n, void* stream) {
  if (n <= 0 || n % 8 != 0 || n / 8 > 0x7fffffffLL * 256 || !y || !h || !al16(y) || !al16(h))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL((k_gelu<false, true>), dim3((unsigned)((n / 8 + 255) / 256)), dim3(256),
                     0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(y),
                     static_cast<const bf16_t*>(nullptr), static_cast<bf16_t*>(h), n / 8);
  return launch_status();
}

int veon_quickgelu_bwd_bf16(const void* dh, const void* y, void* dy, int64_t n,
                            void* stream) {
  if (n <= 0 || n % 8 != 0 || n / 8 > 0x7fffffffLL * 256 || !dh || !y || !dy || !al16(dh) ||
      !al16(y) || !al16(dy))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL((k_gelu<true, true>), dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(y),
                     static_cast<const bf16_t*>(dh), static_cast<bf16_t*>(dy), n / 8);
  return launch_status();
}

int64_t veon_layernorm_f32_bwd_workspace_bytes(int d) {
  if (!ln_width_ok(d)) return -1;
  return (int64_t)kLnBlocks * 2 * d * (int64_t)sizeof(float);
}

int veon_layernorm_f32_bwd(const void* dout, int dout_half, const float* x,
                           const float* gamma, float* dx, float* sums, void* workspace,
                           int64_t workspace_bytes, int T, int d, float eps, void* stream) {
  if (T <= 0 || !ln_width_ok(d) || !dout || !x || !gamma || !dx || !sums || !workspace ||
      dx == dout || dx == x || !al16(dout) || !al16(x) || !al16(gamma) || !al16(dx) ||
      !al16(sums) || !al16(workspace))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_layernorm_f32_bwd_workspace_bytes(d)) return VEON_ERR_WORKSPACE;
  // at least two rounds of rows per workgroup, at most kLnBlocks workgroups
  int rows = (T + kLnBlocks - 1) / kLnBlocks;
  if (rows < 8) rows = 8;
  const int nblocks = (T + rows - 1) / rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  // one 16-byte chunk (two float4) per lane up to 512 channels, two above
#define VEON_LNF_BWD(HALF)                                                                \
  do {                                                                                    \
    if (d <= 512)                                                                         \
      hipLaunchKernelGGL((k_layernorm_f32_bwd<HALF, 1>), dim3(nblocks), dim3(256), 0, s,  \
                         dout, x, gamma, dx, part, T, d, eps, rows);                      \
    else                                                                                  \
      hipLaunchKernelGGL((k_layernorm_f32_bwd<HALF, 2>), dim3(nblocks), dim3(256), 0, s,  \
                         dout, x, gamma, dx, part, T, d, eps, rows);                      \
  } while (0)
  if (dout_half) VEON_LNF_BWD(true); else VEON_LNF_BWD(false);
#undef VEON_LNF_BWD
  const int n4 = 2 * d / 4;
  hipLaunchKernelGGL(k_ln_sums_final, dim3((n4 + 3) / 4), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(part), reinterpret_cast<float4*>(sums),
                     n4, nblocks);
  return launch_status();
}

}  // extern "C"
