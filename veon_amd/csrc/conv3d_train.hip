// Training of the 3x3x3 Conv3d body on the padded channels-last half grid of
// conv3d.hip: the weight gradient on the matrix cores, and train-mode BatchNorm3d
// (batch statistics) as bandwidth passes over the padded rows.
//
// One ConvModule3d in training mode (align_net_occ3d.py:363-399, BN3d with batch
// statistics):
//     y = conv(x, w)                       stored half, halo rows zero
//     mu, var over the N interior voxels;  xhat = (y - mu) * rstd
//     a = relu(gamma * xhat + beta (+ identity))         stored half, halo rows zero
// and backwards, given da:
//     dz = da * [a > 0];  dbeta = sum dz;  dgamma = sum dz * xhat
//     dy = gamma * rstd * (dz - dbeta / N - xhat * dgamma / N)        halo rows zero
//     dx = conv(dy, flip(w))    (veon_conv3d_k3_bf16 on a re-packed weight)
//     dW[co][tap][ci] = sum_rows dy[row][co] * x[row + off(tap)][ci]
//
// Two facts of the padded layout carry all of it:
//  * halo rows of y and dy are ZERO, so per-channel sums over ALL M padded rows are the
//    sums over the interior; only the count N is the interior's.
//  * a filter tap is the constant row offset off(tap) of conv3d.hip's header comment,
//    so the weight gradient is 27 products dy^T . x_shifted contracted over all M
//    padded rows; where row + off leaves the grid it reads guard rows, which are zero
//    (and every product with a halo row of dy is zero anyway).
// The apply passes write zero halo rows themselves (the shift beta would otherwise
// leak into them): their output is the next conv's padded input.
//
// Weight gradient.  Both operands are stored [row][channel] and contracted over the
// ROW index, so both MFMA fragments are transposed reads of a [row][channel] LDS image:
// ds_read_b64_tr_b16 delivers, per 16-lane group, a 4-row x 16-column block with the
// column on the lane.  Which four rows a lane group takes is free as long as both
// operands take the same ones; here group g of a 16-row set takes rows
// 8 (g & 1) + 4 (g >> 1) + 0..3, so that the two blocks of a 32-lane half lie 8 rows
// apart (conflict-free on the swizzled 256-byte rows of wgrad_kernel.h, where the kernel
// lives: conv2d_train.hip instantiates the same body for 3 x 3).  One workgroup = one
// (dz, dy) pair, a 128 x 128 (Cout x Cin) tile and ALL THREE dx taps: the taps read
// rows k - 1, k, k + 1 of ONE x slab, and the dy fragments are reused three times.
// The contraction is split over K; every split writes its fp32 partial tile to a slab
// of the caller's workspace with plain stores, and a second kernel adds the slabs in
// index order: no atomics, bit-reproducible.
//
// Synchronised BN (nn.SyncBatchNorm, veon_amd/sync_bn.py): the same stage one of the sums,
// then an fp64 stage two that writes ONE message stats[2C + 1] (two sums and the local
// count) for the ranks to add, and one coefficient kernel per direction that reads the
// reduced message: k_bn_sums_stats, k_bn_train_coeffs, k_bn_bwd_coeffs below.
#include "mfma_common.h"
#include "wgrad_kernel.h"

namespace {

// ---------------------------------------------------------------- train-mode BatchNorm
constexpr int kBnBlocks = 512;   // partial sums of stage one (upper bound)

struct Half8 { float v[8]; };
__device__ __forceinline__ Half8 load8(const bf16_t* p) {
  const bf16x8 h = *reinterpret_cast<const bf16x8*>(p);
  Half8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o.v[k] = bf2f((bf16_t)h[k]);
  return o;
}
__device__ __forceinline__ void store8(bf16_t* p, const float* v) {
  const uint4 o = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]),
                   pack_bf16(v[6], v[7])};
  *reinterpret_cast<uint4*>(p) = o;
}
__device__ __forceinline__ bool row_interior(int64_t m, int Zp, int Yp, int Xp) {
  const int YX = Yp * Xp;
  const int pl = (int)(m / YX), rem = (int)(m - (int64_t)pl * YX);
  const int y = rem / Xp, xx = rem - y * Xp, z = pl % Zp;
  return z >= 1 && z <= Zp - 2 && y >= 1 && y <= Yp - 2 && xx >= 1 && xx <= Xp - 2;
}

// Stage one of the per-channel sums over all M padded rows (halo rows hold zeros, so
// these ARE the interior's sums).  One lane = 8 channels of a row; a workgroup walks
// its share of the rows, then adds its row-lanes in order and writes
// part[block][2][C].  BWD = false: (sum y, sum y^2); BWD = true: (sum dz, sum dz xhat)
// with dz = da [a > 0], xhat = (y - mean) rstd.
template <bool BWD>
__global__ __launch_bounds__(256) void k_bn_sums(
    const bf16_t* __restrict__ y, const bf16_t* __restrict__ da,
    const bf16_t* __restrict__ a, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part, int64_t M, int C,
    int rows_per_block) {
  __shared__ float red[256 * 16];
  const int lpr = C / 8;                 // lanes per row
  const int rpb = 256 / lpr;             // rows in flight
  const int lr = threadIdx.x / lpr, lc = threadIdx.x % lpr;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { s1[k] = 0.f; s2[k] = 0.f; mu[k] = 0.f; rs[k] = 0.f; }
  if (lr < rpb) {
    if (BWD) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { mu[k] = mean[lc * 8 + k]; rs[k] = rstd[lc * 8 + k]; }
    }
    for (int64_t r = r0 + lr; r < r1; r += rpb) {
      const Half8 vy = load8(y + r * C + lc * 8);
      if (BWD) {
        const Half8 vd = load8(da + r * C + lc * 8);
        const Half8 va = load8(a + r * C + lc * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float dz = va.v[k] > 0.f ? vd.v[k] : 0.f;
          s1[k] += dz;
          s2[k] = fmaf(dz, (vy.v[k] - mu[k]) * rs[k], s2[k]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          s1[k] += vy.v[k];
          s2[k] = fmaf(vy.v[k], vy.v[k], s2[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    red[threadIdx.x * 16 + k] = s1[k];
    red[threadIdx.x * 16 + 8 + k] = s2[k];
  }
  __syncthreads();
  if (lr == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float s = red[lc * 16 + k];
      for (int j = 1; j < rpb; ++j) s += red[(j * lpr + lc) * 16 + k];
      part[((int64_t)blockIdx.x * 2 + (k >> 3)) * C + lc * 8 + (k & 7)] = s;
    }
  }
}

// Stage two: sums[2][C] = part[0] + part[1] + ... in block order
__global__ __launch_bounds__(256) void k_bn_sums_final(const float* __restrict__ part,
                                                       float* __restrict__ sums, int n,
                                                       int nblocks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = part[i];
  for (int b = 1; b < nblocks; ++b) s += part[(int64_t)b * n + i];
  sums[i] = s;
}

// out = act(y * scale + shift (+ identity)) on interior rows, zero on halo rows
template <bool IDENT, bool RELU>
__global__ __launch_bounds__(256) void k_bn_apply(
    const bf16_t* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ shift, const bf16_t* __restrict__ ident,
    bf16_t* __restrict__ out, int64_t M, int C, int Zp, int Yp, int Xp) {
  const int lpr = C / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = i / lpr;
  const int c = (int)(i - m * lpr) * 8;
  if (m >= M) return;
  float v[8];
  if (row_interior(m, Zp, Yp, Xp)) {
    const Half8 vy = load8(y + m * C + c);
    Half8 vi;
    if (IDENT) vi = load8(ident + m * C + c);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = fmaf(vy.v[k], scale[c + k], shift[c + k]);
      if (IDENT) t += vi.v[k];
      v[k] = RELU ? fmaxf(t, 0.f) : t;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.f;
  }
  store8(out + m * C + c, v);
}

// dz = da [a > 0]; dy = ca dz + cb y + cc on interior rows (the closed form of the
// train-mode BN backward with ca = gamma rstd, cb = -gamma rstd^2 dgamma / N,
// cc = -gamma rstd dbeta / N - cb mean), zero on halo rows; dz_out (optional): the
// gradient of the identity branch.
__global__ __launch_bounds__(256) void k_bn_bwd_apply(
    const bf16_t* __restrict__ da, const bf16_t* __restrict__ a,
    const bf16_t* __restrict__ y, const float* __restrict__ ca,
    const float* __restrict__ cb, const float* __restrict__ cc, bf16_t* __restrict__ dy,
    bf16_t* __restrict__ dz_out, int64_t M, int C, int Zp, int Yp, int Xp) {
  const int lpr = C / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = i / lpr;
  const int c = (int)(i - m * lpr) * 8;
  if (m >= M) return;
  float v[8], z[8];
  if (row_interior(m, Zp, Yp, Xp)) {
    const Half8 vd = load8(da + m * C + c);
    const Half8 va = load8(a + m * C + c);
    const Half8 vy = load8(y + m * C + c);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      z[k] = va.v[k] > 0.f ? vd.v[k] : 0.f;
      v[k] = fmaf(ca[c + k], z[k], fmaf(cb[c + k], vy.v[k], cc[c + k]));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = 0.f; z[k] = 0.f; }
  }
  store8(dy + m * C + c, v);
  if (dz_out != nullptr) store8(dz_out + m * C + c, z);
}

bool bn_shape_ok(int B, int C, int Z, int Y, int X) {
  return B > 0 && C > 0 && Z > 0 && Y > 0 && X > 0 && C % 8 == 0 && C <= 2048 &&
         (int64_t)B * (Z + 2) * (Y + 2) * (X + 2) <= 0x3fffffffLL;
}

// ------------------------------------------------- synchronised BN: statistics as a message
// Stage two of the SyncBatchNorm path: stats[o] = sum over the nblocks partials of output
// o (of n2 = 2C, a multiple of 16) in fp64.  A workgroup owns 16 consecutive outputs:
// thread t reads output 16 blockIdx + (t & 15) of the partials (t >> 4) + 0, 16, 32, ...
// (a wave reads four 64-byte runs of consecutive channels per step) and adds them in
// that order; thread (t & 15) then adds the 16 slices through LDS in slice order.  Every
// partial read was written by stage one and every output is stored: nothing depends on
// what the buffers held.  sums32 (optional): the same sums rounded to fp32; stats[n2]: the
// local count.
constexpr int kStatCols = 16, kStatSlices = 16;

__global__ __launch_bounds__(256) void k_bn_sums_stats(const float* __restrict__ part,
                                                       double* __restrict__ stats,
                                                       float* __restrict__ sums32, int n2,
                                                       int nblocks, double count) {
  __shared__ double red[kStatSlices][kStatCols];
  const int col = threadIdx.x % kStatCols, sl = threadIdx.x / kStatCols;
  const int o = blockIdx.x * kStatCols + col;
  double s = 0.0;
  for (int b = sl; b < nblocks; b += kStatSlices) s += (double)part[(int64_t)b * n2 + o];
  red[sl][col] = s;
  __syncthreads();
  if (sl == 0) {
    double t = red[0][col];
#pragma unroll
    for (int j = 1; j < kStatSlices; ++j) t += red[j][col];
    stats[o] = t;
    if (sums32 != nullptr) sums32[o] = (float)t;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[n2] = count;
}

// The C-sized algebra between the sums and the apply pass, one workgroup.  n is the TOTAL
// count (the last element of the reduced buffer).  Every thread reads num_batches_tracked
// before thread 0 stores its increment (one workgroup: the barrier orders them).
__global__ __launch_bounds__(256) void k_bn_train_coeffs(
    const double* __restrict__ stats, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean_offset, double eps,
    double momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
    int64_t* __restrict__ num_batches_tracked, float* __restrict__ mean,
    float* __restrict__ rstd, float* __restrict__ scale, float* __restrict__ shift, int C) {
  const double n = stats[2 * C];
  double f = momentum;
  if (running_mean != nullptr) {
    const int64_t t = *num_batches_tracked + 1;
    if (momentum < 0.0) f = 1.0 / (double)t;
    __syncthreads();
    if (threadIdx.x == 0) *num_batches_tracked = t;
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    const double m = stats[c] / n;
    double var = stats[C + c] / n - m * m;
    var = var > 0.0 ? var : 0.0;
    const double r = 1.0 / sqrt(var + eps);
    const double sc = (double)gamma[c] * r;
    mean[c] = (float)m;
    rstd[c] = (float)r;
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - m * sc);
    if (running_mean != nullptr) {
      const double mo = mean_offset != nullptr ? m + (double)mean_offset[c] : m;
      const double unbiased = var * (n / (n > 1.0 ? n - 1.0 : 1.0));
      running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * mo);
      running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * unbiased);
    }
  }
}

// (ca, cb, cc) of k_bn_bwd_apply from the reduced backward sums and the total count
__global__ __launch_bounds__(256) void k_bn_bwd_coeffs(
    const double* __restrict__ stats, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ ca,
    float* __restrict__ cb, float* __restrict__ cc, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double n = stats[2 * C];
  const double g = gamma[c], mu = mean[c], r = rstd[c];
  const double b = -g * r * r * stats[C + c] / n;
  ca[c] = (float)(g * r);
  cb[c] = (float)b;
  cc[c] = (float)(-g * r * stats[c] / n - b * mu);
}

bool bn_channels_ok(int C) { return C > 0 && C % 8 == 0 && C <= 2048; }

bool bn_sums_args_ok(bool bwd, const void* y, const void* da, const void* a,
                     const float* mean, const float* rstd, const void* workspace, int B,
                     int C, int Z, int Y, int X) {
  return bn_shape_ok(B, C, Z, Y, X) && y && workspace && al16(y) &&
         (!bwd || (da && a && mean && rstd && al16(da) && al16(a)));
}

// Stage one of both directions into `workspace`; -> the number of partials
int bn_sums_stage_one(bool bwd, const void* y, const void* da, const void* a,
                      const float* mean, const float* rstd, void* workspace, int B, int C,
                      int Z, int Y, int X, void* stream) {
  const int64_t M = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  const int rpb = 256 / (C / 8);
  // at least four rounds of rows per workgroup, at most kBnBlocks workgroups
  int64_t rows = (M + kBnBlocks - 1) / kBnBlocks;
  if (rows < 4 * rpb) rows = 4 * rpb;
  const int nblocks = (int)((M + rows - 1) / rows);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const bf16_t* py = static_cast<const bf16_t*>(y);
  if (bwd)
    hipLaunchKernelGGL(k_bn_sums<true>, dim3(nblocks), dim3(256), 0, s, py,
                       static_cast<const bf16_t*>(da), static_cast<const bf16_t*>(a), mean,
                       rstd, part, M, C, (int)rows);
  else
    hipLaunchKernelGGL(k_bn_sums<false>, dim3(nblocks), dim3(256), 0, s, py, nullptr,
                       nullptr, nullptr, nullptr, part, M, C, (int)rows);
  return nblocks;
}

int bn_sums_impl(bool bwd, const void* y, const void* da, const void* a, const float* mean,
                 const float* rstd, float* sums, void* workspace, int B, int C, int Z,
                 int Y, int X, void* stream) {
  if (!bn_sums_args_ok(bwd, y, da, a, mean, rstd, workspace, B, C, Z, Y, X) || !sums)
    return VEON_ERR_BAD_ARG;
  const int nblocks =
      bn_sums_stage_one(bwd, y, da, a, mean, rstd, workspace, B, C, Z, Y, X, stream);
  hipLaunchKernelGGL(k_bn_sums_final, dim3((2 * C + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const float*>(workspace),
                     sums, 2 * C, nblocks);
  return launch_status();
}

int bn_sums_stats_impl(bool bwd, const void* y, const void* da, const void* a,
                       const float* mean, const float* rstd, double* stats, float* sums32,
                       void* workspace, int B, int C, int Z, int Y, int X, void* stream) {
  if (!bn_sums_args_ok(bwd, y, da, a, mean, rstd, workspace, B, C, Z, Y, X) || !stats ||
      !aligned(stats, 8) || (bwd && (!sums32 || !aligned(sums32, 4))))
    return VEON_ERR_BAD_ARG;
  const int nblocks =
      bn_sums_stage_one(bwd, y, da, a, mean, rstd, workspace, B, C, Z, Y, X, stream);
  hipLaunchKernelGGL(k_bn_sums_stats, dim3(2 * C / kStatCols), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const float*>(workspace),
                     stats, sums32, 2 * C, nblocks, (double)((int64_t)B * Z * Y * X));
  return launch_status();
}

}  // namespace

extern "C" {

int64_t veon_conv3d_k3_wgrad_workspace_bytes(int B, int Z, int Y, int X, int Cin,
                                             int Cout) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || Cin <= 0 || Cout <= 0) return -1;
  const int64_t M = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  return wgrad_workspace_bytes<9>(M, veon_conv3d_guard_rows(Y, X), Cin, Cout);
}

int veon_conv3d_k3_wgrad_bf16(const void* dy_padded, const void* x_padded, float* dw,
                              void* workspace, int64_t workspace_bytes, int B, int Z,
                              int Y, int X, int Cin, int Cout, void* stream) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || Cin <= 0 || Cout <= 0) return VEON_ERR_BAD_ARG;
  const int64_t M = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  return wgrad_run<9>(dy_padded, x_padded, dw, workspace, workspace_bytes, M,
                      veon_conv3d_guard_rows(Y, X), Y + 2, X + 2, Cin, Cout, stream);
}

int64_t veon_bn3d_sums_workspace_bytes(int C) {
  if (C <= 0 || C % 8 != 0 || C > 2048) return -1;
  return (int64_t)kBnBlocks * 2 * C * (int64_t)sizeof(float);
}

int veon_bn3d_sums_bf16(const void* y_padded, float* sums, void* workspace, int B, int C,
                        int Z, int Y, int X, void* stream) {
  return bn_sums_impl(false, y_padded, nullptr, nullptr, nullptr, nullptr, sums, workspace,
                      B, C, Z, Y, X, stream);
}

int veon_bn3d_bwd_sums_bf16(const void* da_padded, const void* a_padded,
                            const void* y_padded, const float* mean, const float* rstd,
                            float* sums, void* workspace, int B, int C, int Z, int Y,
                            int X, void* stream) {
  return bn_sums_impl(true, y_padded, da_padded, a_padded, mean, rstd, sums, workspace, B,
                      C, Z, Y, X, stream);
}

int veon_bn3d_sums_stats_bf16(const void* y_padded, double* stats, void* workspace, int B,
                              int C, int Z, int Y, int X, void* stream) {
  return bn_sums_stats_impl(false, y_padded, nullptr, nullptr, nullptr, nullptr, stats,
                            nullptr, workspace, B, C, Z, Y, X, stream);
}

int veon_bn3d_bwd_sums_stats_bf16(const void* da_padded, const void* a_padded,
                                  const void* y_padded, const float* mean,
                                  const float* rstd, double* stats, float* sums,
                                  void* workspace, int B, int C, int Z, int Y, int X,
                                  void* stream) {
  return bn_sums_stats_impl(true, y_padded, da_padded, a_padded, mean, rstd, stats, sums,
                            workspace, B, C, Z, Y, X, stream);
}

int veon_bn_train_coeffs(const double* stats, const float* gamma, const float* beta,
                         const float* mean_offset, double eps, double momentum,
                         float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* mean, float* rstd,
                         float* scale, float* shift, int C, void* stream) {
  const bool any_running = running_mean || running_var || num_batches_tracked;
  const bool all_running = running_mean && running_var && num_batches_tracked;
  if (!bn_channels_ok(C) || !stats || !gamma || !beta || !mean || !rstd || !scale ||
      !shift || !aligned(stats, 8) || !aligned(gamma, 4) || !aligned(beta, 4) ||
      !aligned(mean_offset, 4) || !aligned(mean, 4) || !aligned(rstd, 4) ||
      !aligned(scale, 4) || !aligned(shift, 4) ||
      (any_running && (!all_running || !aligned(running_mean, 4) || !aligned(running_var, 4) ||
                       !aligned(num_batches_tracked, 8))) ||
      !(eps >= 0.0) || !(momentum <= 1.0))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_bn_train_coeffs, dim3(1), dim3(256), 0,
                     static_cast<hipStream_t>(stream), stats, gamma, beta, mean_offset, eps,
                     momentum, running_mean, running_var, num_batches_tracked, mean, rstd,
                     scale, shift, C);
  return launch_status();
}

int veon_bn_bwd_coeffs(const double* stats, const float* gamma, const float* mean,
                       const float* rstd, float* ca, float* cb, float* cc, int C,
                       void* stream) {
  if (!bn_channels_ok(C) || !stats || !gamma || !mean || !rstd || !ca || !cb || !cc ||
      !aligned(stats, 8) || !aligned(gamma, 4) || !aligned(mean, 4) || !aligned(rstd, 4) ||
      !aligned(ca, 4) || !aligned(cb, 4) || !aligned(cc, 4))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_bn_bwd_coeffs, dim3((C + 255) / 256), dim3(256), 0,
                     static_cast<hipStream_t>(stream), stats, gamma, mean, rstd, ca, cb, cc,
                     C);
  return launch_status();
}

int veon_bn3d_apply_bf16(const void* y_padded, const float* scale, const float* shift,
                         const void* ident_padded, void* out_padded, int relu, int B,
                         int C, int Z, int Y, int X, void* stream) {
  if (!bn_shape_ok(B, C, Z, Y, X) || !y_padded || !scale || !shift || !out_padded ||
      !al16(y_padded) || !al16(out_padded) || (ident_padded && !al16(ident_padded)))
    return VEON_ERR_BAD_ARG;
  const int64_t M = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  const int64_t n = M * (C / 8);
  const dim3 grid((unsigned)((n + 255) / 256));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bf16_t* py = static_cast<const bf16_t*>(y_padded);
  const bf16_t* pi = static_cast<const bf16_t*>(ident_padded);
  bf16_t* po = static_cast<bf16_t*>(out_padded);
#define VEON_BN_APPLY(ID, RL)                                                          \
  hipLaunchKernelGGL((k_bn_apply<ID, RL>), grid, dim3(256), 0, s, py, scale, shift, pi, \
                     po, M, C, Z + 2, Y + 2, X + 2)
  if (pi) { if (relu) VEON_BN_APPLY(true, true); else VEON_BN_APPLY(true, false); }
  else    { if (relu) VEON_BN_APPLY(false, true); else VEON_BN_APPLY(false, false); }
#undef VEON_BN_APPLY
  return launch_status();
}

int veon_bn3d_bwd_apply_bf16(const void* da_padded, const void* a_padded,
                             const void* y_padded, const float* ca, const float* cb,
                             const float* cc, void* dy_padded, void* dz_padded, int B,
                             int C, int Z, int Y, int X, void* stream) {
  if (!bn_shape_ok(B, C, Z, Y, X) || !da_padded || !a_padded || !y_padded || !ca || !cb ||
      !cc || !dy_padded || !al16(da_padded) || !al16(a_padded) || !al16(y_padded) ||
      !al16(dy_padded) || (dz_padded && !al16(dz_padded)))
    return VEON_ERR_BAD_ARG;
  const int64_t M = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  const int64_t n = M * (C / 8);
  hipLaunchKernelGGL(k_bn_bwd_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(da_padded),
                     static_cast<const bf16_t*>(a_padded),
                     static_cast<const bf16_t*>(y_padded), ca, cb, cc,
                     static_cast<bf16_t*>(dy_padded), static_cast<bf16_t*>(dz_padded), M, C,
                     Z + 2, Y + 2, X + 2);
  return launch_status();
}

}  // extern "C"
