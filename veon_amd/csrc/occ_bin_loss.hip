// The occupancy term of VEON's training loss from the LOW-resolution logits, forward and
// backward: BCE_BinOcc_Loss (loss/occ_loss_utils/occ3d_nuscenes.py:200-212) on the
// trilinearly upsampled bin_occ (san_in_veon_temporal.py:202-210), i.e.
// F.interpolate(trilinear, align_corners=False) + permute + a weighted two-class
// F.cross_entropy with an ignore index.  The upsampled logits are never stored: the
// forward keeps one fp32 coefficient per output voxel.
//
//   k_bin_fwd     one thread per output voxel in LABEL order (b, x, y, z: z fastest, so
//                 the label reads and the coefficient stores coalesce): both channels
//                 blended from the 8 corners (occ_interp.h's source / blend), nll =
//                 logsumexp - up_t with the maximum subtracted, c = w_t (p_0 - [t == 0])
//                 stored (0 where ignored); per-workgroup fp64 partial sums of
//                 w_t nll and w_t in a fixed order
//   k_bin_reduce  one workgroup adds the partials in a fixed order: loss and 1 / sum w_t
//   k_bin_bwd     (2x per axis) one thread per low-resolution voxel walks its 4x4x4
//                 candidate outputs in a fixed order with occ_interp.h's axis_weight, so
//                 forward and backward agree on every corner by construction; every
//                 element of the (B, 2, z, y, x) gradient is stored, channel 1 = -channel 0
//
// No atomics, no memset, nothing read back; bounds come from the arguments only.  No half
// operands: the file is identical in both library flavours.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_reduce.h"
#include "mfma_common.h"
#include "occ_interp.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

__global__ __launch_bounds__(kBlock) void k_bin_fwd(
    const float* __restrict__ logits, Strides5 ls, Grid g, int64_t total,
    const unsigned char* __restrict__ labels, const float* __restrict__ cw, int ignore_index,
    int free_index, float* __restrict__ coef, double* __restrict__ partials) {
  __shared__ double red[2][kWaves];
  const int64_t n = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double sums[2] = {0.0, 0.0};   // numerator, denominator
  double &num = sums[0], &den = sums[1];
  if (n < total) {
    const int zo = (int)(n % g.Zo);
    const int yo = (int)((n / g.Zo) % g.Yo);
    const int xo = (int)((n / ((int64_t)g.Zo * g.Yo)) % g.Xo);
    const int64_t b = n / ((int64_t)g.Zo * g.Yo * g.Xo);
    const int lab = labels[n];
    float c = 0.f;
    if (lab != ignore_index) {
      const Axis az = source_clamped(zo, g.scz, g.zi), ay = source_clamped(yo, g.scy, g.yi),
                 ax = source_clamped(xo, g.scx, g.xi);
      int64_t off[8];
      corner_offsets(off, ls, az, ay, ax);
      const float* l0 = logits + b * ls.b;
      const float* l1 = l0 + ls.c;
      float v0[8], v1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v0[j] = l0[off[j]];
        v1[j] = l1[off[j]];
      }
      const float u0 = blend(v0, az, ay, ax), u1 = blend(v1, az, ay, ax);
      const int t = lab >= free_index ? 1 : 0;
      const float m = fmaxf(u0, u1);
      const float e0 = expf(u0 - m), e1 = expf(u1 - m);
      const float s = e0 + e1;
      const float nll = (m + logf(s)) - (t ? u1 : u0);
      const float w = cw[t];
      c = w * (e0 / s - (t ? 0.f : 1.f));
      num = (double)w * (double)nll;
      den = (double)w;
    }
    coef[n] = c;
  }
  block_sum(sums, red);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = num;
    partials[2 * (int64_t)blockIdx.x + 1] = den;
  }
}

__global__ __launch_bounds__(kBlock) void k_bin_reduce(const double* __restrict__ partials,
                                                      int64_t count, float* __restrict__ out) {
  __shared__ double red[2][kWaves];
  double sums[2] = {0.0, 0.0};   // numerator, denominator
  double &num = sums[0], &den = sums[1];
  for (int64_t i = threadIdx.x; i < count; i += kBlock) {
    num += partials[2 * i];
    den += partials[2 * i + 1];
  }
  block_sum(sums, red);
  if (threadIdx.x == 0) {
    out[0] = (float)(num / den);                 // nothing counted: 0/0 = NaN, as torch
    out[1] = den > 0.0 ? (float)(1.0 / den) : 0.f;  // ... with an all-zero gradient
  }
}

// Thread j = ((b * xi + ix) * yi + iy) * zi + iz (z fastest: neighbouring threads read
// neighbouring coefficients).  grad: (B, 2, zi, yi, xi) contiguous.
__global__ __launch_bounds__(kBlock) void k_bin_bwd(
    const float* __restrict__ coef, const float* __restrict__ out,
    const float* __restrict__ gout, Grid g, int64_t nlow, float* __restrict__ grad) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= nlow) return;
  const int iz = (int)(j % g.zi);
  const int iy = (int)((j / g.zi) % g.yi);
  const int ix = (int)((j / ((int64_t)g.zi * g.yi)) % g.xi);
  const int64_t b = j / ((int64_t)g.zi * g.yi * g.xi);
  float wz[4], wy[4], wx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wz[k] = axis_weight(2 * iz - 1 + k, g.Zo, iz, g.scz, g.zi);
    wy[k] = axis_weight(2 * iy - 1 + k, g.Yo, iy, g.scy, g.yi);
    wx[k] = axis_weight(2 * ix - 1 + k, g.Xo, ix, g.scx, g.xi);
  }
  const float* cb = coef + b * ((int64_t)g.Xo * g.Yo * g.Zo);
  float acc = 0.f;
  for (int kx = 0; kx < 4; ++kx) {
    if (wx[kx] == 0.f) continue;     // outside the grid, or a tap that does not reach ix
    const int ox = 2 * ix - 1 + kx;
    for (int ky = 0; ky < 4; ++ky) {
      if (wy[ky] == 0.f) continue;
      const int oy = 2 * iy - 1 + ky;
      const float* row = cb + ((int64_t)ox * g.Yo + oy) * g.Zo;
      const float wxy = wx[kx] * wy[ky];
#pragma unroll
      for (int kz = 0; kz < 4; ++kz) {
        if (wz[kz] == 0.f) continue;
        acc += row[2 * iz - 1 + kz] * (wz[kz] * wxy);
      }
    }
  }
  const float v = acc * (gout[0] * out[1]);
  const int64_t plane = (int64_t)g.zi * g.yi * g.xi;
  const int64_t at = ((int64_t)iz * g.yi + iy) * g.xi + ix;
  grad[(b * 2) * plane + at] = v;
  grad[(b * 2 + 1) * plane + at] = -v;
}

// output voxels of (B, Zo, Yo, Xo), or -1 when a 1-D grid of 256-thread workgroups and
// 32-bit axis indices cannot cover them
inline int64_t out_voxels(int B, int Zo, int Yo, int Xo) {
  if (B <= 0 || Zo <= 0 || Yo <= 0 || Xo <= 0) return -1;
  const int64_t lim = 0x7fffffffLL;
  const int64_t zy = (int64_t)Zo * Yo;
  if (zy > lim || zy * Xo > lim || zy * Xo * B > lim) return -1;
  return zy * Xo * B;
}

inline int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

extern "C" int64_t veon_occ_bin_loss_workspace_bytes(int B, int Zo, int Yo, int Xo) {
  const int64_t n = out_voxels(B, Zo, Yo, Xo);
  return n < 0 ? -1 : blocks_of(n) * 2 * (int64_t)sizeof(double);
}

extern "C" int veon_occ_bin_loss_fwd(const float* logits, const int64_t* logit_strides, int B,
                                     int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                     const unsigned char* labels, const float* class_weights,
                                     int ignore_index, int free_index, float* coef,
                                     void* workspace, int64_t workspace_bytes, float* out,
                                     void* stream) {
  const int64_t total = out_voxels(B, Zo, Yo, Xo);
  const int64_t st_ok = logit_strides ? 1 : 0;
  if (total < 0 || !st_ok || zi <= 0 || yi <= 0 || xi <= 0 || !logits || !labels ||
      !class_weights || !coef || !workspace || !out || !aligned(logits, 4) ||
      !aligned(class_weights, 4) || !aligned(coef, 4) || !aligned(out, 4) ||
      !aligned(workspace, 8))
    return VEON_ERR_BAD_ARG;
  const int64_t* st = logit_strides;
  if (st[0] < 0 || st[1] < 0 || st[2] < 0 || st[3] < 0 || st[4] < 0) return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_occ_bin_loss_workspace_bytes(B, Zo, Yo, Xo))
    return VEON_ERR_WORKSPACE;
  const Strides5 ls = strides5(st);
  const Grid g{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
               (float)xi / (float)Xo};
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t nb = blocks_of(total);
  double* partials = static_cast<double*>(workspace);
  hipLaunchKernelGGL(k_bin_fwd, dim3((unsigned)nb), dim3(kBlock), 0, s, logits, ls, g, total,
                     labels, class_weights, ignore_index, free_index, coef, partials);
  hipLaunchKernelGGL(k_bin_reduce, dim3(1), dim3(kBlock), 0, s, partials, nb, out);
  return launch_status();
}

extern "C" int veon_occ_bin_loss_bwd(const float* coef, const float* out, const float* gout,
                                     int B, int zi, int yi, int xi, float* grad,
                                     void* stream) {
  if (zi <= 0 || yi <= 0 || xi <= 0 || zi > (1 << 20) || yi > (1 << 20) || xi > (1 << 20))
    return VEON_ERR_BAD_ARG;
  if (out_voxels(B, 2 * zi, 2 * yi, 2 * xi) < 0 || !coef || !out || !gout || !grad ||
      !aligned(coef, 4) || !aligned(out, 4) || !aligned(gout, 4) || !aligned(grad, 4))
    return VEON_ERR_BAD_ARG;
  const Grid g{zi, yi, xi, 2 * zi, 2 * yi, 2 * xi, 0.5f, 0.5f, 0.5f};
  const int64_t nlow = (int64_t)B * zi * yi * xi;
  hipLaunchKernelGGL(k_bin_bwd, dim3((unsigned)blocks_of(nlow)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), coef, out, gout, g, nlow, grad);
  return launch_status();
}
