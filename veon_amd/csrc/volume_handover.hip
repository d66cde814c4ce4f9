// Hand-over kernels between the padded half rows the prediction heads train on and the
// fp32 channels-last tensors the feature-alignment loss (occ_align_loss.hip) reads and
// returns:
//
//   k_unpack_cl        interior rows of a padded half grid [B][Z+2][Y+2][X+2][Cp] -> a
//                      contiguous fp32 (B, Z, Y, X, C), C <= Cp: no transpose, so the loss
//                      takes its 16-byte path on the result without a copy of its own
//   k_sigm_bwd_pack_cl the backward of f = sigmoid(pre) - 0.5 fused with the pack: an fp32
//                      channels-last gradient d f (any outer strides) and the stored half
//                      f -> d pre = d f (0.25 - f^2) as a whole padded half STORAGE, halo
//                      and guard rows written as zeros (every row is stored: the
//                      destination needs no memset)
//
// One thread per 4 channels of one row.  Bounds come from the arguments only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_common.h"

namespace {

__global__ __launch_bounds__(256) void k_unpack_cl(const bf16_t* __restrict__ in,
                                                   float* __restrict__ out, int64_t total,
                                                   int Cp, int C, int Z, int Y, int X) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = (C + 3) / 4;
  const int c = (int)(idx % c4) * 4;
  int64_t v = idx / c4;                                  // voxel (b, z, y, x)
  const int x = (int)(v % X);
  v /= X;
  const int y = (int)(v % Y);
  v /= Y;
  const int z = (int)(v % Z);
  const int64_t b = v / Z;
  const int64_t row = ((b * (Z + 2) + z + 1) * (Y + 2) + y + 1) * (X + 2) + x + 1;
  const bf16_t* src = in + row * Cp + c;
  float* dst = out + (idx / c4) * C + c;
  if (c + 4 <= C && (C & 3) == 0) {                      // Cp % 4 == 0: 8-byte aligned
    const uint2 q = *reinterpret_cast<const uint2*>(src);
    *reinterpret_cast<float4*>(dst) =
        make_float4(bf2f((bf16_t)(q.x & 0xffff)), bf2f((bf16_t)(q.x >> 16)),
                    bf2f((bf16_t)(q.y & 0xffff)), bf2f((bf16_t)(q.y >> 16)));
  } else {
    for (int e = 0; e < 4 && c + e < C; ++e) dst[e] = bf2f(src[e]);
  }
}

struct Strides4 {
  int64_t b, z, y, x;
};

// rows: all rows of the storage (guard + padded grid + guard); C % 4 == 0
__global__ __launch_bounds__(256) void k_sigm_bwd_pack_cl(
    const float* __restrict__ grad, Strides4 gs, int vec, const bf16_t* __restrict__ f,
    bf16_t* __restrict__ out, int64_t total, int64_t guard, int64_t M, int C, int Z, int Y,
    int X) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c4 = C / 4;
  const int c = (int)(idx % c4) * 4;
  const int64_t srow = idx / c4;                         // row of the storage
  uint2 q = make_uint2(0u, 0u);
  const int64_t r = srow - guard;                        // row of the padded grid
  if (r >= 0 && r < M) {
    int64_t v = r;
    const int xp = (int)(v % (X + 2));
    v /= X + 2;
    const int yp = (int)(v % (Y + 2));
    v /= Y + 2;
    const int zp = (int)(v % (Z + 2));
    const int64_t b = v / (Z + 2);
    if (xp >= 1 && xp <= X && yp >= 1 && yp <= Y && zp >= 1 && zp <= Z) {
      const float* gp = grad + b * gs.b + (zp - 1) * gs.z + (yp - 1) * gs.y + (xp - 1) * gs.x + c;
      float d[4];
      if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(gp);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = gp[e];
      }
      const uint2 fq = *reinterpret_cast<const uint2*>(f + srow * C + c);
      const float fv[4] = {bf2f((bf16_t)(fq.x & 0xffff)), bf2f((bf16_t)(fq.x >> 16)),
                           bf2f((bf16_t)(fq.y & 0xffff)), bf2f((bf16_t)(fq.y >> 16))};
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = d[e] * (0.25f - fv[e] * fv[e]);
      q.x = pack_bf16(d[0], d[1]);
      q.y = pack_bf16(d[2], d[3]);
    }
  }
  *reinterpret_cast<uint2*>(out + srow * C + c) = q;
}

// rows of the padded grid, or -1 when the sizes are not supported
inline int64_t padded_rows(int B, int Z, int Y, int X) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || Z > (1 << 20) || Y > (1 << 20) || X > (1 << 20))
    return -1;
  const int64_t zy = (int64_t)(Z + 2) * (Y + 2);
  if (zy > (1LL << 40) / (X + 2)) return -1;
  const int64_t per = zy * (X + 2);
  if (per > (1LL << 40) / B) return -1;
  return per * B;
}

}  // namespace

extern "C" int veon_volume_unpack_cl_f32(const void* padded, float* out, int B, int Cp, int C,
                                         int Z, int Y, int X, void* stream) {
  const int64_t M = padded_rows(B, Z, Y, X);
  if (M < 0 || !padded || !out || C <= 0 || C > Cp || Cp % 4 != 0 || !aligned(padded, 8) ||
      !aligned(out, 16))
    return VEON_ERR_BAD_ARG;
  const int64_t total = (int64_t)B * Z * Y * X * ((C + 3) / 4);
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_unpack_cl, dim3((unsigned)blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(padded), out,
                     total, Cp, C, Z, Y, X);
  return launch_status();
}

extern "C" int veon_volume_sigm_bwd_pack_cl(const float* grad, const int64_t* grad_strides,
                                            const void* f_storage, void* out_storage,
                                            int64_t guard_rows, int B, int C, int Z, int Y,
                                            int X, void* stream) {
  const int64_t M = padded_rows(B, Z, Y, X);
  if (M < 0 || !grad || !grad_strides || !f_storage || !out_storage || f_storage == out_storage ||
      C <= 0 || C % 4 != 0 || guard_rows != veon_conv3d_guard_rows(Y, X) || !aligned(grad, 4) ||
      !aligned(f_storage, 8) || !aligned(out_storage, 8))
    return VEON_ERR_BAD_ARG;
  const int64_t* st = grad_strides;
  if (st[0] < 0 || st[1] < 0 || st[2] < 0 || st[3] < 0) return VEON_ERR_BAD_ARG;
  // channels-last rows: C may not run past the row into the next voxel
  if (X > 1 && C > st[3]) return VEON_ERR_BAD_ARG;
  const Strides4 gs{st[0], st[1], st[2], st[3]};
  const int vec = aligned(grad, 16) && st[0] % 4 == 0 && st[1] % 4 == 0 && st[2] % 4 == 0 &&
                  st[3] % 4 == 0;
  const int64_t total = (M + 2 * guard_rows) * (C / 4);
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_sigm_bwd_pack_cl, dim3((unsigned)blocks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), grad, gs, vec,
                     static_cast<const bf16_t*>(f_storage), static_cast<bf16_t*>(out_storage),
                     total, guard_rows, M, C, Z, Y, X);
  return launch_status();
}
