// Training of the HSA network's ConvBlock (highres_side_adaptor.py:31-52) on the padded
// channels-last half images of conv3d.hip's 2-D mode:
//     y1 = conv1(a) + b1                      stored half, halo rows zero
//     c  = LN1(GELU(y1))                      stored half, halo rows zero
//     y2 = conv2(c) + b2                      stored half
//     out = LN2(y2) (+ residual)              fp32 tokens (veon_image_layernorm_bf16)
// and backwards, given dout (fp32 tokens):
//     dy2 = LN2'(dout; y2)                    padded half, halo rows zero
//     dW2[co][ky][kx][ci] = sum_rows dy2[row][co] * c[row + off(ky, kx)][ci]
//     dc  = conv(dy2, flip(w2))               (veon_conv2d_k3_bf16 on a re-packed weight)
//     dy1 = LN1'(dc; GELU(y1)) * GELU'(y1)    padded half, halo rows zero
//     dW1 from (dy1, a), da = conv(dy1, flip(w1))
// with the per-channel sums dgamma = sum dout * xhat, dbeta = sum dout and the conv
// bias gradient db = sum dy of each LayerNorm backward pass.
//
// The weight gradient is the kernel of wgrad_kernel.h (shared with conv3d_train.hip) with
// one ky per workgroup: tap (ky, kx) is the row offset (ky - 1)(X + 2) + (kx - 1), the
// three kx taps read rows k - 1, k, k + 1 of one x slab.  Halo rows of dy are zero, so
// the contraction over ALL padded rows is the interior's; where row + off leaves the
// image it reads guard rows, which a PaddedImage allocates as zeros.
//
// The LayerNorm passes keep k_image_layernorm's layout: one wave per padded row, up to
// two 16-byte chunks per lane (C <= 1024), statistics in fp32 and recomputed where
// they are needed (nothing but the half images is stored between forward and backward).
#include "mfma_common.h"
#include "ln_common.h"
#include "wgrad_kernel.h"

namespace {

// ------------------------------------------------------------------ LayerNorm passes
// (GELU and its slope, the lane layout of a row and its statistics: ln_common.h)

// out = LN(GELU(in)) on interior rows, zeros on halo rows
__global__ __launch_bounds__(256) void k_image_gelu_layernorm(
    const bf16_t* __restrict__ in, const float* __restrict__ gamma,
    const float* __restrict__ beta, bf16_t* __restrict__ out, int B, int Y, int X, int C,
    float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int Yp = Y + 2, Xp = X + 2;
  if (m >= (int64_t)B * Yp * Xp) return;
  const int x = (int)(m % Xp), y = (int)((m / Xp) % Yp);
  const int nchunk = C / 8;
  const bool has[2] = {lane < nchunk, lane + 64 < nchunk};
  float v[16];
  if (x >= 1 && x <= X && y >= 1 && y <= Y) {
    load_row<2>(in + m * C, lane, has, v);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float slope;
      gelu_and_slope(v[k], &v[k], &slope);
    }
    float mean, rstd;
    row_stats<2>(v, has, C, eps, &mean, &rstd);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!has[h]) continue;
      const int c0 = (lane + 64 * h) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        v[8 * h + k] = (v[8 * h + k] - mean) * rstd * gamma[c0 + k] + beta[c0 + k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = 0.f;
  }
  store_row<2>(out + m * C, lane, has, v);
}

// LayerNorm backward (optionally through GELU in front of it), stage one of the sums.
// Workgroup b walks padded rows [b rows_per_block, (b + 1) rows_per_block), wave w of it
// rows w, w + 4, ...: per interior row, with u = GELU(x) or x,
//   xhat = (u - mean) rstd,  a = dout gamma,  du = rstd (a - mean(a) - xhat mean(a xhat))
//   dx = du GELU'(x)  or  du
// written as half (halo rows: zeros), and every lane keeps the running sums of its 8 N
// channels: dout xhat, dout, dx (fp32, before dx is rounded).  At the end the four waves
// are added in wave order and part[b][3][C] is written.
template <bool GELU_IN, bool DOUT_TOKENS, int N>
__global__ __launch_bounds__(256) void k_image_layernorm_bwd(
    const void* __restrict__ dout, const bf16_t* __restrict__ xin,
    const float* __restrict__ gamma, bf16_t* __restrict__ dx, float* __restrict__ part,
    int B, int Y, int X, int C, float eps, int rows_per_block) {
  constexpr int E = 8 * N;                 // channels per lane
  __shared__ float red[3][3 * E * 64];     // waves 1..3: [sum * E + k][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Yp = Y + 2, Xp = X + 2;
  const int64_t M = (int64_t)B * Yp * Xp;
  const int nchunk = C / 8;
  const bool has[2] = {lane < nchunk, N == 2 && lane + 64 < nchunk};
  float gm[E], acc[3 * E];
#pragma unroll
  for (int k = 0; k < E; ++k)
    gm[k] = has[k >> 3] ? gamma[(lane + 64 * (k >> 3)) * 8 + (k & 7)] : 0.f;
#pragma unroll
  for (int k = 0; k < 3 * E; ++k) acc[k] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  for (int64_t m = r0 + wave; m < r1; m += 4) {
    const int x = (int)(m % Xp), y = (int)((m / Xp) % Yp), b = (int)(m / ((int64_t)Xp * Yp));
    float u[E], d[E], slope[E];
    (void)b;   // the token index of DOUT_TOKENS only
    if (x >= 1 && x <= X && y >= 1 && y <= Y) {   // wave-uniform
      load_row<N>(xin + m * C, lane, has, u);
      if (DOUT_TOKENS) {
        const float* p = static_cast<const float*>(dout) +
                         (((int64_t)b * Y + (y - 1)) * X + (x - 1)) * C;
#pragma unroll
        for (int h = 0; h < N; ++h) {
          float4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
          if (has[h]) {
            lo = *reinterpret_cast<const float4*>(p + (lane + 64 * h) * 8);
            hi = *reinterpret_cast<const float4*>(p + (lane + 64 * h) * 8 + 4);
          }
          d[8 * h + 0] = lo.x; d[8 * h + 1] = lo.y; d[8 * h + 2] = lo.z; d[8 * h + 3] = lo.w;
          d[8 * h + 4] = hi.x; d[8 * h + 5] = hi.y; d[8 * h + 6] = hi.z; d[8 * h + 7] = hi.w;
        }
      } else {
        load_row<N>(static_cast<const bf16_t*>(dout) + m * C, lane, has, d);
      }
      if (GELU_IN) {
#pragma unroll
        for (int k = 0; k < E; ++k) gelu_and_slope(u[k], &u[k], &slope[k]);
      }
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
        float g = rstd * (d[k] * gm[k] - s1 - u[k] * s2);
        if (GELU_IN) g *= slope[k];
        acc[k] = fmaf(d[k], u[k], acc[k]);
        acc[E + k] += d[k];
        acc[2 * E + k] += g;
        d[k] = g;
      }
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k) d[k] = 0.f;
    }
    store_row<N>(dx + m * C, lane, has, d);
  }
  park_waves<3 * E>(acc, red, lane, wave);
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < 3 * E; ++k) acc[k] = add_waves_in_order(acc[k], red, k * 64 + lane);
    float* o = part + (int64_t)blockIdx.x * 3 * C;
#pragma unroll
    for (int s = 0; s < 3; ++s)
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

bool ln_shape_ok(int B, int C, int Y, int X) {
  return B > 0 && Y > 0 && X > 0 && C > 0 && C % 8 == 0 && C <= 1024 &&
         ((int64_t)B * (Y + 2) * (X + 2) + 3) / 4 <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int64_t veon_conv2d_k3_wgrad_workspace_bytes(int B, int Y, int X, int Cin, int Cout) {
  if (B <= 0 || Y <= 0 || X <= 0 || Cin <= 0 || Cout <= 0) return -1;
  const int64_t M = (int64_t)B * (Y + 2) * (X + 2);
  return wgrad_workspace_bytes<3>(M, veon_conv3d_guard_rows(Y, X), Cin, Cout);
}

int veon_conv2d_k3_wgrad_bf16(const void* dy_padded, const void* x_padded, float* dw,
                              void* workspace, int64_t workspace_bytes, int B, int Y,
                              int X, int Cin, int Cout, void* stream) {
  if (B <= 0 || Y <= 0 || X <= 0 || Cin <= 0 || Cout <= 0) return VEON_ERR_BAD_ARG;
  const int64_t M = (int64_t)B * (Y + 2) * (X + 2);
  return wgrad_run<3>(dy_padded, x_padded, dw, workspace, workspace_bytes, M,
                      veon_conv3d_guard_rows(Y, X), Y + 2, X + 2, Cin, Cout, stream);
}

int veon_image_gelu_layernorm_bf16(const void* in_padded, const float* gamma,
                                   const float* beta, void* out_padded, int B, int C,
                                   int Y, int X, float eps, void* stream) {
  if (!ln_shape_ok(B, C, Y, X) || !in_padded || !gamma || !beta || !out_padded ||
      in_padded == out_padded || !al16(in_padded) || !al16(out_padded))
    return VEON_ERR_BAD_ARG;
  const int64_t M = (int64_t)B * (Y + 2) * (X + 2);
  hipLaunchKernelGGL(k_image_gelu_layernorm, dim3((unsigned)((M + 3) / 4)), dim3(256), 0,
                     static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(in_padded), gamma, beta,
                     static_cast<bf16_t*>(out_padded), B, Y, X, C, eps);
  return launch_status();
}

int64_t veon_image_layernorm_bwd_workspace_bytes(int C) {
  if (C <= 0 || C % 8 != 0 || C > 1024) return -1;
  return (int64_t)kLnBlocks * 3 * C * (int64_t)sizeof(float);
}

int veon_image_layernorm_bwd_bf16(const void* dout, int dout_tokens_f32,
                                  const void* x_padded, int gelu_in, const float* gamma,
                                  void* dx_padded, float* sums, void* workspace,
                                  int64_t workspace_bytes, int B, int C, int Y, int X,
                                  float eps, void* stream) {
  if (!ln_shape_ok(B, C, Y, X) || !dout || !x_padded || !gamma || !dx_padded || !sums ||
      !workspace || dx_padded == dout || dx_padded == x_padded || !al16(dout) ||
      !al16(x_padded) || !al16(dx_padded) || !al16(sums) || !al16(workspace))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_image_layernorm_bwd_workspace_bytes(C)) return VEON_ERR_WORKSPACE;
  const int64_t M = (int64_t)B * (Y + 2) * (X + 2);
  // at least two rounds of rows per workgroup, at most kLnBlocks workgroups
  int64_t rows = (M + kLnBlocks - 1) / kLnBlocks;
  if (rows < 8) rows = 8;
  const int nblocks = (int)((M + rows - 1) / rows);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bf16_t* px = static_cast<const bf16_t*>(x_padded);
  bf16_t* pd = static_cast<bf16_t*>(dx_padded);
  float* part = static_cast<float*>(workspace);
  // one 16-byte chunk per lane up to 512 channels (half the registers), two above
#define VEON_LN_BWD(GE, TK)                                                              \
  do {                                                                                   \
    if (C <= 512)                                                                        \
      hipLaunchKernelGGL((k_image_layernorm_bwd<GE, TK, 1>), dim3(nblocks), dim3(256), 0, \
                         s, dout, px, gamma, pd, part, B, Y, X, C, eps, (int)rows);      \
    else                                                                                 \
      hipLaunchKernelGGL((k_image_layernorm_bwd<GE, TK, 2>), dim3(nblocks), dim3(256), 0, \
                         s, dout, px, gamma, pd, part, B, Y, X, C, eps, (int)rows);      \
  } while (0)
  if (gelu_in) { if (dout_tokens_f32) VEON_LN_BWD(true, true); else VEON_LN_BWD(true, false); }
  else         { if (dout_tokens_f32) VEON_LN_BWD(false, true); else VEON_LN_BWD(false, false); }
#undef VEON_LN_BWD
  const int n4 = 3 * C / 4;
  hipLaunchKernelGGL(k_ln_sums_final, dim3((n4 + 3) / 4), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(part), reinterpret_cast<float4*>(sums),
                     n4, nblocks);
  return launch_status();
}

}  // extern "C"
