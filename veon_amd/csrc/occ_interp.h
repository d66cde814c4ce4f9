// Trilinear source indices, the 8-corner blend and the half-wave reduction shared by
// the kernels that read the LOW-resolution occupancy volume at evaluation-grid voxels
// (occ_retrieval.hip, occ_align_loss.hip): one definition of ATen's source-index rule,
// so that a forward and a backward that use it agree on every corner and weight.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct Strides5 {
  int64_t b, c, z, y, x;
};

struct Axis {
  int i0, i1;
  float l0, l1;
};

// ATen's area_pixel_compute_source_index (align_corners=False, no scale_factor:
// scale = in / out in float), as occ_head.hip; i0 is also clamped at the top, which
// the formula never reaches -- it keeps every read inside the volume by construction
__device__ __forceinline__ Axis source(int dst, float scale, int in_size) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Axis a;
  a.i0 = (int)src;
  a.i0 = a.i0 < in_size - 1 ? a.i0 : in_size - 1;
  a.i1 = a.i0 + (a.i0 < in_size - 1 ? 1 : 0);
  a.l1 = src - (float)a.i0;
  a.l1 = a.l1 < 0.f ? 0.f : (a.l1 > 1.f ? 1.f : a.l1);
  a.l0 = 1.f - a.l1;
  return a;
}

// Weight with which output index o feeds low-resolution index j along one axis (0 for an
// o outside the grid): the transpose of `source`, for the gather-form backwards.  At a
// clamped border both taps land on the same index and their weights add.
__device__ __forceinline__ float axis_weight(int o, int out_size, int j, float scale,
                                             int in_size) {
  if (o < 0 || o >= out_size) return 0.f;
  const Axis a = source(o, scale, in_size);
  return (a.i0 == j ? a.l0 : 0.f) + (a.i1 == j ? a.l1 : 0.f);
}

// v[0..7] = corners (z0y0x0, z0y0x1, z0y1x0, z0y1x1, z1y0x0, ...): ATen's nested blend
__device__ __forceinline__ float blend(const float* v, const Axis& az, const Axis& ay,
                                       const Axis& ax) {
  return az.l0 * (ay.l0 * (ax.l0 * v[0] + ax.l1 * v[1]) +
                  ay.l1 * (ax.l0 * v[2] + ax.l1 * v[3])) +
         az.l1 * (ay.l0 * (ax.l0 * v[4] + ax.l1 * v[5]) +
                  ay.l1 * (ax.l0 * v[6] + ax.l1 * v[7]));
}

// element offsets of the 8 corners (within one batch element and channel)
__device__ __forceinline__ void corner_offsets(int64_t* o, const Strides5& s, const Axis& az,
                                               const Axis& ay, const Axis& ax) {
  const int64_t z0 = az.i0 * s.z, z1 = az.i1 * s.z, y0 = ay.i0 * s.y, y1 = ay.i1 * s.y;
  const int64_t x0 = ax.i0 * s.x, x1 = ax.i1 * s.x;
  o[0] = z0 + y0 + x0; o[1] = z0 + y0 + x1; o[2] = z0 + y1 + x0; o[3] = z0 + y1 + x1;
  o[4] = z1 + y0 + x0; o[5] = z1 + y0 + x1; o[6] = z1 + y1 + x0; o[7] = z1 + y1 + x1;
}

// Sum over the 32 lanes of a half wave; every lane gets the same bits (each step adds
// a lane's value to its partner's in both lanes, and fp32 addition commutes).  DPP
// inside the 16-lane rows (quad xor 1, quad xor 2, half-row mirror, row mirror), then
// v_permlane16_swap pairs rows 0/1 and 2/3 (asm with its wait states, as
// vit_block.hip's max_over_rows).
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

struct Grid {
  int zi, yi, xi, Zo, Yo, Xo;
  float scz, scy, scx;
};

}  // namespace
