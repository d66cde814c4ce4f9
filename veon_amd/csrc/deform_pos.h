// Sample positions of TemporalDeformable's deformable attention
// (mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:138-196), shared by the
// forward gather (temporal.hip) and its backward (temporal_train.hip) so that both
// compute bit-identical positions: the backward re-derives every corner and weight from
// the raw offsets instead of storing them.
#pragma once
#include "mfma_common.h"

namespace {

constexpr int kDeformSamples = 8;

// torch.linspace(-1, 1, n)[i]
__device__ __forceinline__ float deform_base(int i, int n) {
  return n > 1 ? -1.f + 2.f * i / (n - 1) : -1.f;
}

struct DeformPos {
  float o0, o1, o2;   // tanh of the raw offsets
  float fx, fy, fz;   // un-normalised, clamped coordinates along X, Y, Z
  int x0, y0, z0, x1, y1, z1;
  float tx, ty, tz;
};

// One sample of the voxel whose linspace coordinates are (zn, yn, xn); `o` points at its
// three raw offsets.  The reference stacks its base grid (z, y, x) and divides by
// (D, H, W), and grid_sample reads that last axis as (x, y, z): component 0 -- built from
// the z index -- is the position along X, component 2 the one along Z.
__device__ __forceinline__ DeformPos deform_pos(const bf16_t* __restrict__ o, float zn,
                                                float yn, float xn, int Z, int Y, int X) {
  DeformPos p;
  p.o0 = tanhf(bf2f(o[0]));
  p.o1 = tanhf(bf2f(o[1]));
  p.o2 = tanhf(bf2f(o[2]));
  const float gx = fminf(fmaxf(zn + p.o0 / Z, -1.f), 1.f);
  const float gy = fminf(fmaxf(yn + p.o1 / Y, -1.f), 1.f);
  const float gz = fminf(fmaxf(xn + p.o2 / X, -1.f), 1.f);
  p.fx = (gx + 1.f) * 0.5f * (X - 1);
  p.fy = (gy + 1.f) * 0.5f * (Y - 1);
  p.fz = (gz + 1.f) * 0.5f * (Z - 1);
  p.x0 = min((int)floorf(p.fx), X - 1);
  p.y0 = min((int)floorf(p.fy), Y - 1);
  p.z0 = min((int)floorf(p.fz), Z - 1);
  p.tx = p.fx - p.x0;
  p.ty = p.fy - p.y0;
  p.tz = p.fz - p.z0;
  p.x1 = min(p.x0 + 1, X - 1);
  p.y1 = min(p.y0 + 1, Y - 1);
  p.z1 = min(p.z0 + 1, Z - 1);
  return p;
}

}  // namespace
