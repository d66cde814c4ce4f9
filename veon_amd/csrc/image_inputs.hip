// Camera inputs of VEON on MI355X: PrepareImageInputs (mmdet3d/datasets/pipelines/
// loading.py:1073-1329) from decoded uint8 frames: Pillow's 8-bit bicubic `Image.resize`
// bit for bit, the crop window, the optional mirror, the normalised fp32 planes, and the
// depthanythingv2 tail of the depth branch.
//
// Pillow's resampling (ImagingResample, 8 bits per channel) is integer arithmetic on tables
// that depend on the two sizes alone: per output index a first tap and a tap count
// (`bounds`) and 22-bit fixed-point coefficients (`kk`), made on the host
// (veon_amd/image_inputs.py resize_coeffs).  One pass is
//     ss = 2^21 + sum_t pixel[first + t] * kk[t];   out = clamp(ss >> 22, 0, 255)
// in 32-bit integers; the horizontal pass comes first and is rounded to a byte.
//
//   k_resample_h         one thread per pixel of the intermediate: only the rows the
//                        vertical pass of the windows reads
//   k_resample_v_finish  one thread per pixel of the window: the vertical pass, the column
//                        mirror, the uint8 window and the fp32 planes through a table
//                        lut[3][256] of a byte (both imnormalize variants and midas are
//                        functions of a byte: exact by construction, no division here)
//   k_resample_v_finish4 the same, four pixels per thread with dword loads and stores and
//                        float4 stores, where the host has proven the alignment
//   k_cubic_norm         swap, / 255, the four-tap cubic (A = -0.75, rows first, then
//                        columns, taps clamped to the image), (x - mean) / std, in fp32
//
// The tap count is a run-time value of the table (33 at 8:1).  Pixels are three bytes and
// not dword aligned: byte loads, byte stores, ordinary dword stores of the planes, wider
// ones only in k_resample_v_finish4.  Every
// element of every output is written; no memset, no atomics, no hidden copy.  The same code
// in both library flavours (no half operands); -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_common.h"

namespace {
constexpr int kBlock = 256;
constexpr int kPrecisionBits = 22;             // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int clip8(int ss) {
  return min(max(ss >> kPrecisionBits, 0), 255);   // arithmetic shift, as Pillow's clip8
}

// grid (ceil(Wo / 256), rows, BN).  tmp[bn][r][x][c] = horizontal pass of source row
// row0 + r.  The table's first tap and count are clamped to the row, so a wrong table
// cannot read outside the frame.
__global__ __launch_bounds__(kBlock) void k_resample_h(
    const uint8_t* __restrict__ src, int H, int W, int Wo, int row0, int rows,
    const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
    uint8_t* __restrict__ tmp) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= Wo) return;
  const int r = blockIdx.y;
  const int64_t bn = blockIdx.z;
  const int first = min(max(bounds[2 * x], 0), W);
  const int n = min(min(bounds[2 * x + 1], ksize), W - first);
  const int* k = kk + (int64_t)x * ksize;
  const uint8_t* p = src + ((bn * H + row0 + r) * W + first) * 3;
  int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
  for (int t = 0; t < n; ++t) {
    const int w = k[t];
    s0 += (int)p[3 * t] * w;
    s1 += (int)p[3 * t + 1] * w;
    s2 += (int)p[3 * t + 2] * w;
  }
  uint8_t* o = tmp + ((bn * rows + r) * Wo + x) * 3;
  o[0] = (uint8_t)clip8(s0);
  o[1] = (uint8_t)clip8(s1);
  o[2] = (uint8_t)clip8(s2);
}

// grid (ceil(fW / 256), fH, BN).  src holds rows row0 .. row0 + Hs - 1 of the horizontally
// resized image, Ws pixels wide.  bounds == nullptr: no vertical pass, window row y is
// source row y0 + y.
__global__ __launch_bounds__(kBlock) void k_resample_v_finish(
    const uint8_t* __restrict__ src, int Hs, int Ws, int row0,
    const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
    veon_image_windows win, int fH, int fW, const float* __restrict__ lut, int swap,
    uint8_t* __restrict__ canvas, float* __restrict__ planes) {
  const int x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= fW) return;
  const int y = blockIdx.y;
  const int64_t bn = blockIdx.z;
  const int cam = (int)(bn % win.n);
  const int xs = win.x0[cam] + (win.flip[cam] ? fW - 1 - x : x);
  const int ys = win.y0[cam] + y;
  const uint8_t* img = src + bn * Hs * Ws * 3;
  int v0, v1, v2;
  if (bounds) {
    const int first = min(max(bounds[2 * ys] - row0, 0), Hs);
    const int n = min(min(bounds[2 * ys + 1], ksize), Hs - first);
    const int* k = kk + (int64_t)ys * ksize;
    const uint8_t* p = img + ((int64_t)first * Ws + xs) * 3;
    const int64_t step = (int64_t)Ws * 3;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t, p += step) {
      const int w = k[t];
      s0 += (int)p[0] * w;
      s1 += (int)p[1] * w;
      s2 += (int)p[2] * w;
    }
    v0 = clip8(s0);
    v1 = clip8(s1);
    v2 = clip8(s2);
  } else {
    const uint8_t* p = img + ((int64_t)(ys - row0) * Ws + xs) * 3;
    v0 = p[0];
    v1 = p[1];
    v2 = p[2];
  }
  const int64_t pix = (bn * fH + y) * fW + x;
  if (canvas) {
    uint8_t* o = canvas + pix * 3;
    o[0] = (uint8_t)v0;
    o[1] = (uint8_t)v1;
    o[2] = (uint8_t)v2;
  }
  if (planes) {
    // output channel c reads input channel 2 - c under the reference's channel swap
    const int64_t plane = (int64_t)fH * fW;
    float* o = planes + bn * 3 * plane + (int64_t)y * fW + x;
    o[0] = lut[swap ? v2 : v0];
    o[plane] = lut[256 + v1];
    o[2 * plane] = lut[512 + (swap ? v0 : v2)];
  }
}

// The same for four window pixels (12 bytes) per thread, where the host has proven that
// every group of four starts on a dword: fW, Ws and every x0 multiples of four, src and
// canvas dword aligned, planes 16-byte aligned.  Three dword loads per tap instead of twelve
// byte loads, three dword stores of the window, three float4 stores of the planes; the
// table is read from LDS.  grid (ceil(fH * fW / 4 / 256), 1, BN).
__global__ __launch_bounds__(kBlock) void k_resample_v_finish4(
    const uint8_t* __restrict__ src, int Hs, int Ws, int row0,
    const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
    veon_image_windows win, int fH, int fW, const float* __restrict__ lut, int swap,
    uint8_t* __restrict__ canvas, float* __restrict__ planes) {
  __shared__ float s_lut[768];
  if (planes) {
    for (int i = threadIdx.x; i < 768; i += kBlock) s_lut[i] = lut[i];
    __syncthreads();
  }
  const int groups = fW >> 2;
  const int g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= fH * groups) return;
  const int y = g / groups, x = (g - y * groups) << 2;
  const int64_t bn = blockIdx.z;
  const int cam = (int)(bn % win.n);
  const bool flip = win.flip[cam] != 0;
  const int xs = win.x0[cam] + (flip ? fW - 4 - x : x);
  const int ys = win.y0[cam] + y;
  const uint8_t* img = src + bn * Hs * Ws * 3;
  int v[12];                                     // v[3 i + c]: pixel xs + i, channel c
  if (bounds) {
    const int first = min(max(bounds[2 * ys] - row0, 0), Hs);
    const int n = min(min(bounds[2 * ys + 1], ksize), Hs - first);
    const int* k = kk + (int64_t)ys * ksize;
    const uint32_t* p =
        reinterpret_cast<const uint32_t*>(img + ((int64_t)first * Ws + xs) * 3);
    const int64_t step = (int64_t)Ws * 3 / 4;    // dwords per row
    for (int j = 0; j < 12; ++j) v[j] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t, p += step) {
      const int w = k[t];
      for (int d = 0; d < 3; ++d) {
        const uint32_t word = p[d];
        for (int b = 0; b < 4; ++b) v[4 * d + b] += (int)((word >> (8 * b)) & 0xffu) * w;
      }
    }
    for (int j = 0; j < 12; ++j) v[j] = clip8(v[j]);
  } else {
    const uint32_t* p =
        reinterpret_cast<const uint32_t*>(img + ((int64_t)(ys - row0) * Ws + xs) * 3);
    for (int d = 0; d < 3; ++d) {
      const uint32_t word = p[d];
      for (int b = 0; b < 4; ++b) v[4 * d + b] = (int)((word >> (8 * b)) & 0xffu);
    }
  }
  if (flip) {                                    // pixel i <-> pixel 3 - i
    for (int c = 0; c < 3; ++c) {
      int s = v[c];
      v[c] = v[9 + c];
      v[9 + c] = s;
      s = v[3 + c];
      v[3 + c] = v[6 + c];
      v[6 + c] = s;
    }
  }
  const int64_t pix = (bn * fH + y) * fW + x;
  if (canvas) {
    uint32_t* o = reinterpret_cast<uint32_t*>(canvas + pix * 3);
    for (int d = 0; d < 3; ++d)
      o[d] = (uint32_t)v[4 * d] | (uint32_t)v[4 * d + 1] << 8 | (uint32_t)v[4 * d + 2] << 16 |
             (uint32_t)v[4 * d + 3] << 24;
  }
  if (planes) {
    const int64_t plane = (int64_t)fH * fW;
    float* o = planes + bn * 3 * plane + (int64_t)y * fW + x;
    for (int c = 0; c < 3; ++c) {
      const int ci = swap ? 2 - c : c;
      const float* l = s_lut + 256 * c;
      *reinterpret_cast<float4*>(o + c * plane) =
          make_float4(l[v[ci]], l[v[3 + ci]], l[v[6 + ci]], l[v[9 + ci]]);
    }
  }
}

// OpenCV's cubic coefficients (A = -0.75) of the fraction t, fp32, in its operation order
__device__ __forceinline__ void cubic_weights(float t, float* w) {
  const float A = -0.75f;
  w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
  w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  const float u = 1.f - t;
  w[2] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  w[3] = 1.f - w[0] - w[1] - w[2];
}

struct Norm3 {
  float mean[3], std[3];
};

// grid (ceil(ow / 256), oh, BN)
__global__ __launch_bounds__(kBlock) void k_cubic_norm(
    const uint8_t* __restrict__ src, int h, int w, int oh, int ow, double scale_y,
    double scale_x, int swap, Norm3 norm, float* __restrict__ out) {
  const int dx = blockIdx.x * kBlock + threadIdx.x;
  if (dx >= ow) return;
  const int dy = blockIdx.y;
  const int64_t bn = blockIdx.z;
  float fx = (float)((dx + 0.5) * scale_x - 0.5);
  float fy = (float)((dy + 0.5) * scale_y - 0.5);
  const int sx = (int)floorf(fx), sy = (int)floorf(fy);
  fx -= (float)sx;
  fy -= (float)sy;
  float wx[4], wy[4];
  cubic_weights(fx, wx);
  cubic_weights(fy, wy);
  int xi[4];
  for (int k = 0; k < 4; ++k) xi[k] = min(max(sx - 1 + k, 0), w - 1) * 3;
  const uint8_t* img = src + bn * h * w * 3;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int r = 0; r < 4; ++r) {
    const uint8_t* row = img + (int64_t)min(max(sy - 1 + r, 0), h - 1) * w * 3;
    for (int c = 0; c < 3; ++c) {
      const int ci = swap ? 2 - c : c;
      const float hr = (float)row[xi[0] + ci] / 255.f * wx[0] +
                       (float)row[xi[1] + ci] / 255.f * wx[1] +
                       (float)row[xi[2] + ci] / 255.f * wx[2] +
                       (float)row[xi[3] + ci] / 255.f * wx[3];
      acc[c] = r == 0 ? hr * wy[0] : acc[c] + hr * wy[r];
    }
  }
  const int64_t plane = (int64_t)oh * ow;
  float* o = out + bn * 3 * plane + (int64_t)dy * ow + dx;
  for (int c = 0; c < 3; ++c) o[c * plane] = (acc[c] - norm.mean[c]) / norm.std[c];
}

inline bool grid_ok(int64_t bn, int rows) {
  return bn > 0 && bn <= 65535 && rows > 0 && rows <= 65535;
}
}  // namespace

extern "C" {

int veon_image_resample_h(const uint8_t* frames, int BN, int H, int W, int Wo, int row0,
                          int rows, const int* bounds, const int* kk, int ksize,
                          uint8_t* tmp, void* stream) {
  if (!frames || !tmp || !bounds || !kk || H <= 0 || W <= 0 || Wo <= 0 || ksize <= 0 ||
      row0 < 0 || rows <= 0 || (int64_t)row0 + rows > H || !grid_ok(BN, rows))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_resample_h, dim3((Wo + kBlock - 1) / kBlock, rows, BN), dim3(kBlock),
                     0, static_cast<hipStream_t>(stream), frames, H, W, Wo, row0, rows,
                     bounds, kk, ksize, tmp);
  return launch_status();
}

int veon_image_resample_v_finish(const uint8_t* src, int BN, int Hs, int Ws, int row0,
                                 int Ho, const int* bounds, const int* kk, int ksize,
                                 veon_image_windows win, int fH, int fW, const float* lut,
                                 int swap, uint8_t* canvas, float* planes, void* stream) {
  if (!src || Hs <= 0 || Ws <= 0 || row0 < 0 || Ho <= 0 || fH <= 0 || fW <= 0 ||
      (!canvas && !planes) || (planes && !lut) || !grid_ok(BN, fH))
    return VEON_ERR_BAD_ARG;
  if (bounds ? (!kk || ksize <= 0) : ((int64_t)row0 + Hs > Ho)) return VEON_ERR_BAD_ARG;
  if (win.n <= 0 || win.n > VEON_IMAGE_MAX_WINDOWS) return VEON_ERR_BAD_ARG;
  // four pixels per thread only where every group of four provably starts on a dword
  bool by_four = fW % 4 == 0 && Ws % 4 == 0 && aligned(src, 4) &&
                 (!canvas || aligned(canvas, 4)) && (!planes || aligned(planes, 16)) &&
                 (int64_t)fH * (fW / 4) <= 0x7fffffffLL;
  for (int i = 0; i < win.n; ++i) {
    // the window lies inside the resized image; without a vertical pass also inside src
    if (win.x0[i] < 0 || win.y0[i] < 0 || (int64_t)win.x0[i] + fW > Ws ||
        (int64_t)win.y0[i] + fH > Ho)
      return VEON_ERR_BAD_ARG;
    if (!bounds && (win.y0[i] < row0 || (int64_t)win.y0[i] + fH > (int64_t)row0 + Hs))
      return VEON_ERR_BAD_ARG;
    by_four = by_four && win.x0[i] % 4 == 0;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (by_four) {
    const int64_t groups = (int64_t)fH * (fW / 4);
    hipLaunchKernelGGL(k_resample_v_finish4, dim3((unsigned)((groups + kBlock - 1) / kBlock), 1, BN),
                       dim3(kBlock), 0, st, src, Hs, Ws, row0, bounds, kk, ksize, win, fH, fW,
                       lut, swap, canvas, planes);
  } else {
    hipLaunchKernelGGL(k_resample_v_finish, dim3((fW + kBlock - 1) / kBlock, fH, BN),
                       dim3(kBlock), 0, st, src, Hs, Ws, row0, bounds, kk, ksize, win, fH, fW,
                       lut, swap, canvas, planes);
  }
  return launch_status();
}

int veon_image_cubic_norm(const uint8_t* src, int BN, int h, int w, int oh, int ow, int swap,
                          float mean0, float mean1, float mean2, float std0, float std1,
                          float std2, float* out, void* stream) {
  if (!src || !out || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || !grid_ok(BN, oh) ||
      !(std0 != 0.f) || !(std1 != 0.f) || !(std2 != 0.f))
    return VEON_ERR_BAD_ARG;
  const Norm3 norm = {{mean0, mean1, mean2}, {std0, std1, std2}};
  hipLaunchKernelGGL(k_cubic_norm, dim3((ow + kBlock - 1) / kBlock, oh, BN), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), src, h, w, oh, ow, (double)h / oh,
                     (double)w / ow, swap, norm, out);
  return launch_status();
}

}  // extern "C"
