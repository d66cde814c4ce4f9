// Source indices, corner offsets and the 8-corner blend of the occupancy path's tail,
// shared by the kernel that writes the upsampled volumes (occ_head.hip) and the
// label-only kernel (occ_eval.hip): one definition, so that the two produce the same
// label bit for bit (the library is built without FMA contraction).
//
// Interpolation follows ATen's upsample_trilinear3d (area_pixel_compute_source_index
// with align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0, the nested
// w/h/t blend).
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

// the eight corner offsets (elements, within one batch element and channel) of a
// voxel; 32-bit: the host checks the extent
struct Corners {
  int o[8];
};

__device__ __forceinline__ Corners corners(const Strides5& s, const Axis& az,
                                           const Axis& ay, const Axis& ax) {
  const int z0 = az.i0 * (int)s.z, z1 = az.i1 * (int)s.z;
  const int y0 = ay.i0 * (int)s.y, y1 = ay.i1 * (int)s.y;
  const int x0 = ax.i0 * (int)s.x, x1 = ax.i1 * (int)s.x;
  return Corners{{z0 + y0 + x0, z0 + y0 + x1, z0 + y1 + x0, z0 + y1 + x1,
                  z1 + y0 + x0, z1 + y0 + x1, z1 + y1 + x0, z1 + y1 + x1}};
}

__device__ __forceinline__ float blend(const float* __restrict__ p, const Corners& k,
                                       const Axis& az, const Axis& ay, const Axis& ax) {
  return az.l0 * (ay.l0 * (ax.l0 * p[k.o[0]] + ax.l1 * p[k.o[1]]) +
                  ay.l1 * (ax.l0 * p[k.o[2]] + ax.l1 * p[k.o[3]])) +
         az.l1 * (ay.l0 * (ax.l0 * p[k.o[4]] + ax.l1 * p[k.o[5]]) +
                  ay.l1 * (ax.l0 * p[k.o[6]] + ax.l1 * p[k.o[7]]));
}

// Both kernels take the VEC4 (channels-last, 16-byte rows) instantiation on the same
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
