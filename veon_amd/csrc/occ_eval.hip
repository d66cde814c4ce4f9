// On-device Occ3D evaluation (Metric_mIoU, mmdet3d/datasets/occ_metrics.py:78-147): the
// confusion matrix of label volumes that already exist.  The label-only tails of the
// occupancy path, which can add the same matrix while they write their labels, are in
// occ_tail.hip; the LDS counters both use are in occ_label_tile.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occ_label_tile.h"

namespace {

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

}  // namespace

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
