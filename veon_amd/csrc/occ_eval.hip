// On-device Occ3D evaluation (Metric_mIoU, mmdet3d/datasets/occ_metrics.py:78-147):
// the label-only tail of the occupancy path with the confusion matrix fused in, and the
// same confusion matrix for label volumes that already exist.
//
// k_occ_labels computes what k_occ_classify (occ_head.hip) computes per voxel -- the
// same source indices, corner offsets, blend nest and class loop (occ_interp.h), so the
// same label bit for bit -- and writes NOTHING but the uint8 label volume (B,Xo,Yo,Zo)
// that VEONTemporal.simple_test returns (detectors/veon_temporal.py:219-241): 640 KB
// at the VEON shape instead of 48 MB of upsampled logits and 5 MB of int64 labels.
//
// Mapping, LDS staging, W-byte output and the histogram's LDS counters: occ_label_tile.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occ_interp.h"
#include "occ_label_tile.h"

namespace {

// The label of output voxel (b, z, y, x): k_occ_classify without its stores.
template <bool VEC4>
__device__ __forceinline__ int label_of(const float* __restrict__ sem, const Strides5& ss,
                                        int Q, const float* __restrict__ bin,
                                        const Strides5& bs, const Geometry& g, int b, int z,
                                        int y, int x) {
  const Axis az = source(z, g.scz, g.zi), ay = source(y, g.scy, g.yi),
             ax = source(x, g.scx, g.xi);
  float vmax = -INFINITY;
  int cls = 0;
  bool bad = false;
  const float* sp = sem + b * ss.b;
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
      // Every value is needed here, also those of the surplus floats past class Q - 1:
      // without the stores of k_occ_classify the compiler otherwise computes them under
      // the branch below, splits each 16-byte load into three and waits for each part.
#pragma unroll
      for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(val4[e]));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (c + e < Q) {
          const float val = val4[e];
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
  const float om = o0 > o1 ? o0 : o1;
  const float e0 = expf(o0 - om), e1 = expf(o1 - om);
  const bool keep = scored && (e0 / (e0 + e1) > 0.5f);
  return keep ? cls : Q;
}

template <bool VEC4, int W>
__global__ __launch_bounds__(THREADS) void k_occ_labels(
    const float* __restrict__ sem, Strides5 ss, int Q, const float* __restrict__ bin,
    Strides5 bs, int B, Geometry g, int TY, uint8_t* __restrict__ labels,
    const uint8_t* __restrict__ gt, const uint8_t* __restrict__ mask,
    unsigned long long* __restrict__ hist) {
  extern __shared__ __align__(16) unsigned char smem[];
  label_tiles<W>(
      smem,
      [&](int b, int z, int y, int x) {
        return label_of<VEC4>(sem, ss, Q, bin, bs, g, b, z, y, x);
      },
      Q + 1, B, g, TY, labels, gt, mask, hist);
}

__device__ __forceinline__ bool count_one(unsigned* cnt, int n_cl, int64_t p, unsigned gv,
                                          unsigned mv) {
  if (!mv || gv >= (unsigned)n_cl) return false;
  if ((uint64_t)p >= (uint64_t)n_cl) return true;   // in no bin
  atomicAdd(cnt + gv * n_cl + (int)p, 1u);
  return false;
}

// P: the label type (uint8_t or int64_t); E voxels per lane and step (4: gt and mask,
// and uint8 labels, as one 4-byte load each)
template <typename P, int E>
__global__ __launch_bounds__(THREADS) void k_confusion(
    const P* __restrict__ pred, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, int64_t n, int n_cl,
    unsigned long long* __restrict__ hist, int* __restrict__ flag) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned* cnt = reinterpret_cast<unsigned*>(smem);
  zero_counters(cnt, n_cl);
  __syncthreads();
  bool bad = false;
  const int64_t groups = (n + E - 1) / E;
  for (int64_t grp = (int64_t)blockIdx.x * THREADS + threadIdx.x; grp < groups;
       grp += (int64_t)gridDim.x * THREADS) {
    const int64_t base = grp * E;
    if (E == 4 && base + 4 <= n) {
      const uint32_t gv = *reinterpret_cast<const uint32_t*>(gt + base);
      const uint32_t mv = mask ? *reinterpret_cast<const uint32_t*>(mask + base) : ~0u;
      int64_t p[4];
      if (sizeof(P) == 1) {
        const uint32_t pv = *reinterpret_cast<const uint32_t*>(pred + base);
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (pv >> (8 * j)) & 0xffu;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = (int64_t)pred[base + j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bad |= count_one(cnt, n_cl, p[j], (gv >> (8 * j)) & 0xffu, (mv >> (8 * j)) & 0xffu);
    } else {
      const int64_t end = base + E < n ? base + E : n;
      for (int64_t i = base; i < end; ++i)
        bad |= count_one(cnt, n_cl, (int64_t)pred[i], gt[i], mask ? mask[i] : 1u);
    }
  }
  if (bad && flag) *flag = 1;
  __syncthreads();
  flush_counters(cnt, n_cl, hist);
}

template <bool VEC4>
void launch_labels(int W, int blocks, size_t lds, hipStream_t st, const float* sem,
                   const Strides5& ss, int Q, const float* bin, const Strides5& bs, int B,
                   const Geometry& g, int TY, uint8_t* labels, const uint8_t* gt,
                   const uint8_t* mask, unsigned long long* hist) {
#define VEON_LABELS(w)                                                                   \
  hipLaunchKernelGGL((k_occ_labels<VEC4, w>), dim3((unsigned)blocks), dim3(THREADS), lds, \
                     st, sem, ss, Q, bin, bs, B, g, TY, labels, gt, mask, hist)
  switch (W) {
    case 16: VEON_LABELS(16); break;
    case 8: VEON_LABELS(8); break;
    case 4: VEON_LABELS(4); break;
    default: VEON_LABELS(1); break;
  }
#undef VEON_LABELS
}

}  // namespace

extern "C" int veon_occ_labels(const float* sem, const int64_t* sem_strides, int Q,
                               const float* bin, const int64_t* bin_strides, int B, int zi,
                               int yi, int xi, int Zo, int Yo, int Xo, uint8_t* labels,
                               const uint8_t* gt, const uint8_t* mask, int64_t* hist,
                               void* stream) {
  if (!sem || !bin || !sem_strides || !bin_strides || !labels || Q <= 0 || Q > 254 ||
      B <= 0 || zi <= 0 || yi <= 0 || xi <= 0 || Zo <= 0 || Yo <= 0 || Xo <= 0 ||
      Zo > MAX_ZO)
    return VEON_ERR_BAD_ARG;
  // the histogram needs the ground truth and the other way round; a mask needs both
  if ((gt != nullptr) != (hist != nullptr) || (mask && !gt)) return VEON_ERR_BAD_ARG;
  if (hist && Q + 1 > MAX_CL) return VEON_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * Zo * Yo * Xo;
  if (total > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  if (!strides_fit(sem_strides, zi, yi, xi) || !strides_fit(bin_strides, zi, yi, xi))
    return VEON_ERR_BAD_ARG;
  const Strides5 ss = strides5(sem_strides), bs = strides5(bin_strides);
  // ATen: scale = in / out in float (area_pixel_compute_scale, no scale_factor given)
  const Geometry g{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
                   (float)xi / (float)Xo};
  const TileLaunch t = tile_launch(B, Zo, Yo, Xo, Q + 1, labels, gt, mask, hist != nullptr);
  const int TY = t.TY, W = t.W, blocks = t.blocks;
  const size_t lds = t.lds;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  if (vec4_rows(sem, ss, Q))
    launch_labels<true>(W, blocks, lds, st, sem, ss, Q, bin, bs, B, g, TY, labels, gt, mask, h);
  else
    launch_labels<false>(W, blocks, lds, st, sem, ss, Q, bin, bs, B, g, TY, labels, gt, mask, h);
  return launch_status();
}

extern "C" int veon_occ_confusion(const void* pred, int pred_elem_bytes, const uint8_t* gt,
                                  const uint8_t* mask, int64_t n, int n_cl, int64_t* hist,
                                  int* flag, void* stream) {
  if (!pred || !gt || !hist || (pred_elem_bytes != 1 && pred_elem_bytes != 8) || n <= 0 ||
      n > 0x7fffffffLL || n_cl <= 0 || n_cl > MAX_CL || !aligned(pred, pred_elem_bytes))
    return VEON_ERR_BAD_ARG;
  const bool quads = aligned(gt, 4) && aligned(mask, 4) &&
                     (pred_elem_bytes == 8 || aligned(pred, 4));
  const int64_t groups = quads ? (n + 3) / 4 : n;
  int64_t blocks = (groups + THREADS - 1) / THREADS;
  blocks = blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks;
  const size_t lds = sizeof(unsigned) * n_cl * n_cl;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
#define VEON_CONFUSION(P, E)                                                              \
  hipLaunchKernelGGL((k_confusion<P, E>), dim3((unsigned)blocks), dim3(THREADS), lds, st, \
                     static_cast<const P*>(pred), gt, mask, n, n_cl, h, flag)
  if (pred_elem_bytes == 1) {
    if (quads) VEON_CONFUSION(uint8_t, 4); else VEON_CONFUSION(uint8_t, 1);
  } else {
    if (quads) VEON_CONFUSION(int64_t, 4); else VEON_CONFUSION(int64_t, 1);
  }
#undef VEON_CONFUSION
  return launch_status();
}
