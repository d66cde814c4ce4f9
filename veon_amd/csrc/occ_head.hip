// Tail of the occupancy path in one pass (SANInVeonTemporal.forward,
// san_in_veon_temporal.py:196-211, and VEONTemporal.simple_test,
// detectors/veon_temporal.py:219-227): trilinear upsampling (align_corners=False)
// of the class logits and of the two occupancy logits from the head's grid to the
// evaluation grid, softmax over the classes -> best class, softmax over
// (occupied, free) -> keep, class-or-free label written in the (X, Y, Z) order of
// the benchmark.
//
// The reference runs this as ~10 tensor ops over 48 MB of fp32 outputs; here every
// output element is written once and nothing else touches HBM (the 6 MB of
// low-resolution logits stay in L2): the kernel is bound by its output writes.
// One lane = one output voxel, x fastest: every channel plane is written
// coalesced; the 8-byte labels go out transposed (strided), 5 MB in all.
//
// Interpolation follows ATen's upsample_trilinear3d (area_pixel_compute_source_index
// with align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0, the nested
// w/h/t blend); the label is the first maximum of the class logits (= of their
// softmax, up to ties at rounding level).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occ_interp.h"
#include "host_common.h"

namespace {

// VEC4: the class logits are channels-last (channel stride 1, rows 16-byte aligned,
// at least 4*ceil(Q/4) floats per row): four classes per 16-byte corner load -- the
// kernel is bound by the number of cache lines its gathers touch, 3.4x fewer so.
template <bool VEC4>
__global__ __launch_bounds__(256) void k_occ_classify(
    const float* __restrict__ sem, Strides5 ss, int Q, const float* __restrict__ bin,
    Strides5 bs, int B, int zi, int yi, int xi, int Zo, int Yo, int Xo, float scz,
    float scy, float scx, float* __restrict__ sem_out, float* __restrict__ bin_out,
    int64_t* __restrict__ cls_out) {
  // 32-bit index arithmetic (the host checks B*Zo*Yo*Xo < 2^31): 64-bit divisions
  // cost ~100 VGPRs here
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;
  const unsigned plane32 = (unsigned)Zo * Yo * Xo;
  if (idx >= (unsigned)B * plane32) return;
  const int b = (int)(idx / plane32);
  const unsigned v = idx - (unsigned)b * plane32;
  const int x = (int)(v % (unsigned)Xo);
  const int y = (int)((v / (unsigned)Xo) % (unsigned)Yo);
  const int z = (int)(v / ((unsigned)Xo * Yo));
  const int64_t plane = plane32;
  const Axis az = source(z, scz, zi), ay = source(y, scy, yi), ax = source(x, scx, xi);

  // One pass over the classes (a rolled loop: unrolled, the 8 x Q corner loads are
  // all hoisted and the kernel drops to one wave per SIMD with scratch).  The best
  // class of softmax(sem) is the first maximum of the logits; its probability
  // 1 / sum(exp(v - vmax)) is positive exactly when the logits hold no NaN and the
  // maximum is finite (otherwise ATen's softmax is NaN and `score > 0` is false).
  float vmax = -INFINITY;
  int cls = 0;
  bool bad = false;
  const float* sp = sem + b * ss.b;
  float* so = sem_out + (int64_t)b * Q * plane + v;
  int ks[8];
  corner_offsets(ks, ss, az, ay, ax);
  if (VEC4) {
#pragma unroll 1
    for (int c = 0; c < Q; c += 4) {
      float4 k4[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) k4[q] = *reinterpret_cast<const float4*>(sp + c + ks[q]);
      float val4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float k8[8];   // channel c + e of the eight corners
#pragma unroll
        for (int q = 0; q < 8; ++q) k8[q] = reinterpret_cast<const float*>(&k4[q])[e];
        val4[e] = blend(k8, az, ay, ax);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e < Q) {
          const float val = val4[e];
          so[(int64_t)(c + e) * plane] = val;
          bad |= val != val;
          if (val > vmax) {
            vmax = val;
            cls = c + e;
          }
        }
      }
    }
  } else {
#pragma unroll 2
    for (int c = 0; c < Q; ++c) {
      const float val = blend(sp + c * ss.c, ks, az, ay, ax);
      so[(int64_t)c * plane] = val;
      bad |= val != val;
      if (val > vmax) {
        vmax = val;
        cls = c;
      }
    }
  }
  const bool scored = !bad && vmax < INFINITY && vmax > -INFINITY;
  const float* bp = bin + b * bs.b;
  int kb[8];
  corner_offsets(kb, bs, az, ay, ax);
  const float o0 = blend(bp, kb, az, ay, ax), o1 = blend(bp + bs.c, kb, az, ay, ax);
  bin_out[((int64_t)b * 2 + 0) * plane + v] = o0;
  bin_out[((int64_t)b * 2 + 1) * plane + v] = o1;
  const float om = o0 > o1 ? o0 : o1;
  const float e0 = expf(o0 - om), e1 = expf(o1 - om);
  const bool keep = scored && (e0 / (e0 + e1) > 0.5f);
  cls_out[(((int64_t)b * Xo + x) * Yo + y) * Zo + z] = keep ? cls : Q;
}

}  // namespace

extern "C" int veon_occ_classify(const float* sem, const int64_t* sem_strides, int Q,
                                 const float* bin, const int64_t* bin_strides, int B,
                                 int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                 float* sem_out, float* bin_out, int64_t* cls_out,
                                 void* stream) {
  if (!sem || !bin || !sem_strides || !bin_strides || !sem_out || !bin_out || !cls_out ||
      Q <= 0 || B <= 0 || zi <= 0 || yi <= 0 || xi <= 0 || Zo <= 0 ||
      Yo <= 0 || Xo <= 0)
    return VEON_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * Zo * Yo * Xo;
  const int64_t blocks = (total + 255) / 256;
  if (total > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  if (!strides_fit(sem_strides, zi, yi, xi) || !strides_fit(bin_strides, zi, yi, xi))
    return VEON_ERR_BAD_ARG;
  const Strides5 ss = strides5(sem_strides), bs = strides5(bin_strides);
  // ATen: scale = in / out in float (area_pixel_compute_scale, no scale_factor given)
  const float scz = (float)zi / (float)Zo, scy = (float)yi / (float)Yo,
              scx = (float)xi / (float)Xo;
  if (vec4_rows(sem, ss, Q))
    hipLaunchKernelGGL(k_occ_classify<true>, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sem, ss, Q, bin, bs, B, zi, yi,
                       xi, Zo, Yo, Xo, scz, scy, scx, sem_out, bin_out, cls_out);
  else
    hipLaunchKernelGGL(k_occ_classify<false>, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sem, ss, Q, bin, bs, B, zi, yi,
                       xi, Zo, Yo, Xo, scz, scy, scx, sem_out, bin_out, cls_out);
  return launch_status();
}
