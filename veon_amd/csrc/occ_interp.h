// Trilinear sampling of the LOW-resolution occupancy volumes at evaluation-grid voxels:
// source indices, corner offsets and the 8-corner blend, one definition each, shared by
// the occupancy tail (occ_tail.hip: the labels of its four kernels agree bit for bit with
// each other and with ATen; the library is built without FMA contraction) and by retrieval and
// the losses (occ_retrieval.hip, occ_align_loss.hip, occ_bin_loss.hip: a forward and a
// backward that use it agree on every corner and weight).
//
// Interpolation follows ATen's upsample_trilinear3d (area_pixel_compute_source_index
// with align_corners=False and no scale_factor: scale = in / out in float,
// src = scale*(dst+0.5)-0.5 clamped at 0, the nested w/h/t blend).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct Strides5 {
  int64_t b, c, z, y, x;
};

inline Strides5 strides5(const int64_t* st) {
  return Strides5{st[0], st[1], st[2], st[3], st[4]};
}

struct Axis {
  int i0, i1;
  float l0, l1;
};

// The low-resolution and the evaluation grid with the scale of each axis: in / out in
// float, as ATen's area_pixel_compute_scale without a scale_factor.
struct Grid {
  int zi, yi, xi, Zo, Yo, Xo;
  float scz, scy, scx;
};

inline Grid grid_of(int zi, int yi, int xi, int Zo, int Yo, int Xo) {
  return Grid{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
              (float)xi / (float)Xo};
}

// Two source rules, on purpose.  `source` is ATen's, operation for operation: the tail's
// labels must match ATen bit for bit.  `source_clamped` also clamps i0 at the top and l1
// to [0, 1], which the formula never reaches: retrieval and the losses keep every read
// inside the volume by construction.  The clamps cost instructions even where they never
// bind, so neither rule is written on top of the other.
__device__ __forceinline__ Axis source(int dst, float scale, int in_size) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Axis a;
  a.i0 = (int)src;
  a.i1 = a.i0 + (a.i0 < in_size - 1 ? 1 : 0);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.f - a.l1;
  return a;
}

__device__ __forceinline__ Axis source_clamped(int dst, float scale, int in_size) {
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
// o outside the grid): the transpose of `source_clamped`, for the gather-form backwards.
// At a clamped border both taps land on the same index and their weights add.
__device__ __forceinline__ float axis_weight(int o, int out_size, int j, float scale,
                                             int in_size) {
  if (o < 0 || o >= out_size) return 0.f;
  const Axis a = source_clamped(o, scale, in_size);
  return (a.i0 == j ? a.l0 : 0.f) + (a.i1 == j ? a.l1 : 0.f);
}

// Element offsets of the 8 corners (z0y0x0, z0y0x1, z0y1x0, z0y1x1, z1y0x0, ...) within
// one batch element and channel.  O = int where the host has checked the extent
// (strides_fit), int64_t elsewhere.
template <typename O>
__device__ __forceinline__ void corner_offsets(O* o, const Strides5& s, const Axis& az,
                                               const Axis& ay, const Axis& ax) {
  const O z0 = az.i0 * (O)s.z, z1 = az.i1 * (O)s.z, y0 = ay.i0 * (O)s.y, y1 = ay.i1 * (O)s.y;
  const O x0 = ax.i0 * (O)s.x, x1 = ax.i1 * (O)s.x;
  o[0] = z0 + y0 + x0; o[1] = z0 + y0 + x1; o[2] = z0 + y1 + x0; o[3] = z0 + y1 + x1;
  o[4] = z1 + y0 + x0; o[5] = z1 + y0 + x1; o[6] = z1 + y1 + x0; o[7] = z1 + y1 + x1;
}

// ATen's nested blend of the corners p[o[0..7]] (in the order of corner_offsets)
template <typename O>
__device__ __forceinline__ float blend(const float* __restrict__ p, const O* o,
                                       const Axis& az, const Axis& ay, const Axis& ax) {
  return az.l0 * (ay.l0 * (ax.l0 * p[o[0]] + ax.l1 * p[o[1]]) +
                  ay.l1 * (ax.l0 * p[o[2]] + ax.l1 * p[o[3]])) +
         az.l1 * (ay.l0 * (ax.l0 * p[o[4]] + ax.l1 * p[o[5]]) +
                  ay.l1 * (ax.l0 * p[o[6]] + ax.l1 * p[o[7]]));
}

// the same of corner values v[0..7] already in registers
__device__ __forceinline__ float blend(const float* v, const Axis& az, const Axis& ay,
                                       const Axis& ax) {
  constexpr int at[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  return blend(v, at, az, ay, ax);
}

// The tail's kernels take the VEC4 (channels-last, 16-byte rows) instantiation on the same
// condition: at least 4*ceil(Q/4) floats per row, every stride and the base a multiple
// of 16 bytes.
inline bool vec4_rows(const float* sem, const Strides5& ss, int Q) {
  const int q4 = (Q + 3) / 4 * 4;
  return ss.c == 1 && (reinterpret_cast<uintptr_t>(sem) & 15u) == 0 && ss.b % 4 == 0 &&
         ss.z % 4 == 0 && ss.y % 4 == 0 && ss.x % 4 == 0 && ss.x >= q4;
}

// 32-bit corner offsets: every stride non-negative and the far corner below 2^31
inline bool strides_fit(const int64_t* st, int zi, int yi, int xi) {
  return st[2] >= 0 && st[3] >= 0 && st[4] >= 0 &&
         st[2] * (zi - 1) + st[3] * (yi - 1) + st[4] * (xi - 1) <= 0x7fffffffLL;
}

}  // namespace
