// LiDAR depth labels of VEON's depth pre-training stage on MI355X: PointToMultiViewDepth
// (mmdet3d/datasets/pipelines/loading.py:735-759 points2depthmap, :811-821 the projection)
// as the exact per-pixel minimum.
//
// The reference projects the sweep into every camera on the host, sorts the kept points by
// the fp32 key `rank + depth / 100`, keeps the first of each pixel and ships six 512 x 1408
// maps to the device; the loss then takes their block-minimum by 16.  Above rank 2^19 that
// key cannot tell depths 6.25 m apart, so an unstable sort picks the label.  Here
// the nearest return per pixel, or per block x block pixels, is formed where it is used:
//
//   k_lidar_fill      every word of out = 0xffffffff (no caller memset)
//   k_lidar_scatter   one thread per point; the point is read once and projected into the
//                     N cameras of its sample (matrices wave-uniform); a kept depth is
//                     positive, so its bit pattern orders as its value and an unsigned
//                     atomic minimum on out's own storage is exact in any point order
//   k_lidar_finish    0xffffffff -> 0.0f
//
// No float atomics, no workspace, nothing read back.  fp32, one rounding per operation in
// the reference's order (-ffp-contract=off); the same code in both library flavours.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_common.h"

namespace {
constexpr int kBlock = 256;
constexpr unsigned kEmpty = 0xffffffffu;       // above the bits of every positive float

__global__ __launch_bounds__(kBlock) void k_lidar_fill(unsigned* __restrict__ out,
                                                        int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < total) out[i] = kEmpty;
}

__global__ __launch_bounds__(kBlock) void k_lidar_finish(unsigned* __restrict__ out,
                                                          int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < total && out[i] == kEmpty) out[i] = 0u;
}

// grid (ceil(P / 256), B).  Hb x Wb is the output map, H x W the pixel grid it covers in
// blocks of 1 << bshift.
__global__ __launch_bounds__(kBlock) void k_lidar_scatter(
    const float* __restrict__ points, int P, int64_t row_stride,
    const float* __restrict__ lidar2img, const float* __restrict__ post_rots,
    const float* __restrict__ post_trans, int N, float fH, float fW, float fds, int bshift,
    int Hb, int Wb, float lo, float hi, unsigned* __restrict__ out) {
  const int p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= P) return;
  const int b = blockIdx.y;
  const float* pt = points + ((int64_t)b * P + p) * row_stride;
  const float px = pt[0], py = pt[1], pz = pt[2];
  for (int n = 0; n < N; ++n) {
    const int64_t bn = (int64_t)b * N + n;
    float u = px, v = py, d = pz;
    if (lidar2img) {
      const float* M = lidar2img + bn * 12;    // rows of 4: R | t (:814-815)
      const float qx = (M[0] * px + M[1] * py + M[2] * pz) + M[3];
      const float qy = (M[4] * px + M[5] * py + M[6] * pz) + M[7];
      const float qz = (M[8] * px + M[9] * py + M[10] * pz) + M[11];
      const float iu = qx / qz, iv = qy / qz;  // :816-818
      const float* R = post_rots + bn * 9;     // the full 3 x 3 (:819-820)
      const float* T = post_trans + bn * 3;
      u = (R[0] * iu + R[1] * iv + R[2] * qz) + T[0];
      v = (R[3] * iu + R[4] * iv + R[5] * qz) + T[1];
      d = (R[6] * iu + R[7] * iv + R[8] * qz) + T[2];
    }
    // torch.round is round-half-to-even; every test in floating point, so NaN, +-inf and
    // 1e30 fail a comparison before any conversion (:738-743)
    const float x = rintf(u / fds), y = rintf(v / fds);
    const bool kept = x >= 0.f && x < fW && y >= 0.f && y < fH && d < hi && d >= lo;
    if (!kept) continue;
    const int ix = (int)x >> bshift, iy = (int)y >> bshift;   // -0.0f -> pixel 0
    atomicMin(out + (bn * Hb + iy) * Wb + ix, __float_as_uint(d));
  }
}

inline int block_shift(int block) {
  switch (block) {
    case 1: return 0;
    case 2: return 1;
    case 4: return 2;
    case 8: return 3;
    case 16: return 4;
    default: return -1;
  }
}
}  // namespace

extern "C" {

int veon_lidar_depth_render(const float* points, int B, int P, int row_stride,
                            const float* lidar2img, const float* post_rots,
                            const float* post_trans, int N, int H, int W, int downsample,
                            int block, float lo, float hi, float* out, void* stream) {
  const int bshift = block_shift(block);
  if (B <= 0 || B > 65535 || P < 0 || row_stride < 3 || N <= 0 || H <= 0 || W <= 0 ||
      H > (1 << 24) || W > (1 << 24) || downsample <= 0 || bshift < 0 || H % block ||
      W % block || !(lo > 0.f) || !(hi > lo) || !out || (P > 0 && !points))
    return VEON_ERR_BAD_ARG;
  if (lidar2img ? (!post_rots || !post_trans) : N != 1) return VEON_ERR_BAD_ARG;
  const int Hb = H / block, Wb = W / block;
  const int64_t total = (int64_t)B * N * Hb * Wb;
  const int64_t blocks = (total + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL || (int64_t)B * P > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned* words = reinterpret_cast<unsigned*>(out);
  hipLaunchKernelGGL(k_lidar_fill, dim3((unsigned)blocks), dim3(kBlock), 0, st, words, total);
  if (P > 0)
    hipLaunchKernelGGL(k_lidar_scatter, dim3((unsigned)(((int64_t)P + kBlock - 1) / kBlock), B),
                       dim3(kBlock), 0, st, points, P, (int64_t)row_stride, lidar2img,
                       post_rots, post_trans, N, (float)H, (float)W, (float)downsample,
                       bshift, Hb, Wb, lo, hi, words);
  hipLaunchKernelGGL(k_lidar_finish, dim3((unsigned)blocks), dim3(kBlock), 0, st, words,
                     total);
  return launch_status();
}

}  // extern "C"
