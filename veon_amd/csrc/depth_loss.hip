// Depth pre-training loss of VEON's first training stage on MI355X, forward and backward:
// VeonDepthPretrain.forward_train (mmdet3d/models/detectors/veon_depth_pretrain.py:128-154)
// = downsample_depth of the prediction and of the LiDAR depth, the mean-absolute-error
// statistic and LSSViewTransformerRaw.get_depth_loss_own(zoe, ce)
// (mmdet3d/models/necks/view_transformer_raw.py:393-404, 497-535).
//
// The reference selects rows with two boolean masks, reads a scalar back and divides by
// max(1.0, fg_mask.sum()): four host synchronisations and several dozen launches around
// (rows, D+1) intermediates.  Here: three kernels, no atomics, no memset, nothing read back.
//
//   k_depth_loss_rows    one wave per output pixel ("row"): block-min of the prediction
//                        with the winning pixel, block-min of the label, the log
//                        difference, the two-hot BCE value and its derivative with respect
//                        to the block-min; one 32-byte record per row, nothing of size
//                        rows x (D+1) reaches memory
//   k_depth_loss_reduce  one workgroup: fixed-order fp64 sums over the records (mean, then
//                        the unbiased variance about it), the three scalars and the
//                        coefficients of the backward
//   k_depth_loss_bwd     one wave per row: every pixel of the row's block of the gradient
//                        map is stored, the row gradient on the winner, 0 elsewhere
//
// fp32 throughout (the same code in both library flavours).  Sums run in a fixed order:
// repeated calls are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_common.h"
#include "lane_reduce.h"

namespace {
constexpr int kWave = 64;
constexpr int kRowBlock = 256;                 // 4 rows per workgroup
constexpr int kRowsPerBlock = kRowBlock / kWave;
constexpr int kReduceBlock = 512;
constexpr int kReduceWaves = kReduceBlock / kWave;
constexpr int kRec = VEON_DEPTH_LOSS_REC;      // floats per row record
constexpr float kValidBelow = 9225.f;          // :505
constexpr float kAlpha = 1e-7f;                // :508
constexpr float kMinGap = -16.f;               // :420

// record words
enum { R_G = 0, R_ABS = 1, R_BCE = 2, R_FLAGS = 3, R_D = 4, R_T = 5, R_DBCE = 6, R_WIN = 7 };
// coefficient words (floats)
enum { C_MEAN = 0, C_A = 1, C_B = 2, C_CE = 3, C_N = 4, C_NFG = 5, C_SQRT = 6, C_CLIPPED = 7 };

// -gamma * |d - c_k|, clamped below at -16 (forward value of the straight-through clamp)
__device__ __forceinline__ float clamped_gap(float d, float c, float gamma) {
  float gap = -fabsf(d - c) * gamma;
  if (!(gap >= kMinGap)) gap = kMinGap;
  return gap;
}

__global__ __launch_bounds__(kRowBlock) void k_depth_loss_rows(
    const float* __restrict__ depth, const float* __restrict__ gt, int64_t rows, int h, int w,
    int sp, int sg, int D, float step, float off, float gamma, float* __restrict__ rec) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;                     // whole waves leave; no barrier below
  const int x = (int)(row % w);
  const int y = (int)((row / w) % h);
  const int64_t bn = row / ((int64_t)w * h);

  // ---- block-min of the prediction, first pixel in (dy, dx) order on ties
  const int Wp = w * sp;
  const float* src = depth + (bn * h * sp + (int64_t)y * sp) * Wp + (int64_t)x * sp;
  float best = INFINITY;
  int besti = 0x7fffffff;
  bool best_zero = false;
  for (int i = lane; i < sp * sp; i += kWave) {
    const float raw = src[(int64_t)(i / sp) * Wp + (i % sp)];
    const float v = raw == 0.0f ? 1e5f : raw;
    if (v < best) {
      best = v;
      besti = i;
      best_zero = raw == 0.0f;
    }
  }
  float d = best;
  int win = besti;
  // (arg-min with its index as payload: no shared helper)
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(d, o, kWave);
    const int oi = __shfl_xor(win, o, kWave);
    if (ov < d || (ov == d && oi < win)) {
      d = ov;
      win = oi;
    }
  }
  // the lane that owns the winner knows whether it was a zero read as 1e5
  const int win_zero = __shfl((int)(best_zero && besti == win), win & (kWave - 1), kWave);

  // ---- block-min of the label
  const int Wg = w * sg;
  const float* lsrc = gt + (bn * h * sg + (int64_t)y * sg) * Wg + (int64_t)x * sg;
  float t = INFINITY;
  for (int i = lane; i < sg * sg; i += kWave) {
    float v = lsrc[(int64_t)(i / sg) * Wg + (i % sg)];
    if (v == 0.0f) v = 1e5f;
    t = v < t ? v : t;
  }
  // (a min by compare and select, as the serial loop above: no shared helper)
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(t, o, kWave);
    t = ov < t ? ov : t;
  }

  // ---- label bin: argmax_k -|min(t, 500) - c_k|, first index on ties (:439-452);
  //      and the largest gap of the prediction
  const float tc = fminf(t, 500.f);
  float lbest = -INFINITY, mx = -INFINITY;
  int kstar = 0x7fffffff;
  for (int k = lane; k <= D; k += kWave) {
    const float c = (float)k * step + off;
    const float lv = -fabsf(tc - c);
    if (lv > lbest) {
      lbest = lv;
      kstar = k;
    }
    mx = fmaxf(mx, clamped_gap(d, c, gamma));
  }
  // (arg-max with its index as payload: no shared helper)
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const float ov = __shfl_xor(lbest, o, kWave);
    const int ok = __shfl_xor(kstar, o, kWave);
    if (ov > lbest || (ov == lbest && ok < kstar)) {
      lbest = ov;
      kstar = ok;
    }
  }
  mx = wave_max(mx);
  const bool fg = kstar < D;

  // ---- softmax denominator
  float part = 0.f;
  for (int k = lane; k <= D; k += kWave)
    part += expf(clamped_gap(d, (float)k * step + off, gamma) - mx);
  const float sum = wave_sum(part);

  // ---- BCE value, and S = sum_j p_j e_j with e = (p - y) / max(p (1 - p), 1e-12)
  //      (binary_cross_entropy's backward), e_D = 0 for the dropped bin
  float lpart = 0.f, spart = 0.f;
  for (int k = lane; k < D; k += kWave) {
    const float p = expf(clamped_gap(d, (float)k * step + off, gamma) - mx) / sum;
    const float yk = k == kstar ? 1.f : 0.f;
    lpart -= k == kstar ? fmaxf(logf(p), -100.f) : fmaxf(log1pf(-p), -100.f);
    spart += p * ((p - yk) / fmaxf(p * (1.f - p), 1e-12f));
  }
  const float bce = wave_sum(lpart);
  const float S = wave_sum(spart);

  // ---- d(row)/dd = sum_k p_k (e_k - S) * (-gamma sign(d - c_k)): the straight-through
  //      clamp passes the slope on every bin, clamped ones included
  float dpart = 0.f;
  for (int k = lane; k <= D; k += kWave) {
    const float c = (float)k * step + off;
    const float p = expf(clamped_gap(d, c, gamma) - mx) / sum;
    float e = 0.f;
    if (k < D) e = (p - (k == kstar ? 1.f : 0.f)) / fmaxf(p * (1.f - p), 1e-12f);
    const float sgn = d > c ? 1.f : (d < c ? -1.f : 0.f);
    dpart += p * (e - S) * (-gamma * sgn);
  }
  const float dbce = wave_sum(dpart);

  if (lane == 0) {
    const bool valid = t < kValidBelow;
    float4 a, b;
    a.x = logf(d + kAlpha) - logf(t + kAlpha);
    a.y = fabsf(d - t);
    a.z = fg ? bce : 0.f;
    a.w = __int_as_float((valid ? 1 : 0) | (fg ? 2 : 0));
    b.x = d;
    b.y = t;
    b.z = fg ? dbce : 0.f;
    b.w = __int_as_float((win & 0xff) | (win_zero ? 0x100 : 0) | ((kstar < D ? kstar : D) << 16));
    float4* o = reinterpret_cast<float4*>(rec + row * kRec);
    o[0] = a;
    o[1] = b;
  }
}

// One workgroup.  Thread i takes rows i, i + 512, ... in fp64, the waves' shuffle sums meet
// in LDS in wave order: a fixed order.  Pass 2 (squares about the mean) re-reads the
// records, which the first pass left in L2.
__global__ __launch_bounds__(kReduceBlock) void k_depth_loss_reduce(
    const float* __restrict__ rec, int64_t rows, float* __restrict__ out,
    float* __restrict__ coef) {
  __shared__ double red[5][kReduceWaves];
  const int tid = threadIdx.x;
  const float4* r4 = reinterpret_cast<const float4*>(rec);

  double sg = 0.0, sabs = 0.0, sbce = 0.0;
  int nvalid = 0, nfg = 0;
#pragma unroll 4
  for (int64_t r = tid; r < rows; r += kReduceBlock) {
    const float4 a = r4[r * 2];
    const int flags = __float_as_int(a.w);
    if (flags & 1) {
      sg += (double)a.x;
      sabs += (double)a.y;
      ++nvalid;
    }
    if (flags & 2) {
      sbce += (double)a.z;
      ++nfg;
    }
  }
  // the counts as doubles: exact (rows < 2^31)
  double tot[5] = {sg, sabs, sbce, (double)nvalid, (double)nfg};
  block_sum(tot, red);
  const double tg = tot[0], tabs = tot[1], tbce = tot[2], n = tot[3], n_fg = tot[4];
  const double mean = tg / n;                  // n = 0: NaN, as the mean of nothing
  __syncthreads();                             // red[] is reused below

  double ss[1] = {0.0};
#pragma unroll 4
  for (int64_t r = tid; r < rows; r += kReduceBlock) {
    const float4 a = r4[r * 2];
    if (__float_as_int(a.w) & 1) {
      const double dv = (double)a.x - mean;
      ss[0] += dv * dv;
    }
  }
  block_sum(ss, red);
  if (tid == 0) {
    const double tss = ss[0];
    const double var = tss / (n - 1.0);        // n = 1: 0/0 = NaN, as torch.var
    const double Dg = var + 0.15 * mean * mean;
    const double sq = sqrt(Dg);
    const bool clipped = sq > 2.0;             // a NaN is not clipped: it propagates
    const double inv_fg = 1.0 / (n_fg > 1.0 ? n_fg : 1.0);
    out[0] = (float)(clipped ? 2.0 : sq);
    out[1] = (float)(tbce * inv_fg * 0.05);
    out[2] = (float)(tabs / n);
    coef[C_MEAN] = (float)mean;
    coef[C_A] = clipped ? 0.f : (float)(1.0 / ((n - 1.0) * sq));
    coef[C_B] = clipped ? 0.f : (float)(0.15 * mean / (n * sq));
    coef[C_CE] = (float)(0.05 * inv_fg);
    coef[C_N] = (float)n;
    coef[C_NFG] = (float)n_fg;
    coef[C_SQRT] = (float)sq;
    coef[C_CLIPPED] = clipped ? 1.f : 0.f;
  }
}

// Every pixel of the (BN, h*sp, w*sp) gradient map is stored once: the row's gradient
//   g_zoe * [(g - m) a + b] / (d + 1e-7)  (valid rows)  +  g_ce * 0.05/max(1, n_fg) * dbce
// (foreground rows) on the winning pixel unless that pixel was a zero, 0 elsewhere.
__global__ __launch_bounds__(kRowBlock) void k_depth_loss_bwd(
    const float* __restrict__ rec, const float* __restrict__ coef,
    const float* __restrict__ g_zoe, const float* __restrict__ g_ce, int64_t rows, int h,
    int w, int sp, float* __restrict__ grad) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int x = (int)(row % w);
  const int y = (int)((row / w) % h);
  const int64_t bn = row / ((int64_t)w * h);
  const float4* r4 = reinterpret_cast<const float4*>(rec + row * kRec);
  const float4 a = r4[0], b = r4[1];
  const int flags = __float_as_int(a.w), packed = __float_as_int(b.w);
  float r = 0.f;
  if (g_zoe && (flags & 1) && coef[C_CLIPPED] == 0.f)
    r += *g_zoe * (((a.x - coef[C_MEAN]) * coef[C_A] + coef[C_B]) / (b.x + kAlpha));
  if (g_ce && (flags & 2)) r += *g_ce * (coef[C_CE] * b.z);
  const int win = (packed & 0x100) ? -1 : (packed & 0xff);
  const int Wp = w * sp;
  float* dst = grad + (bn * h * sp + (int64_t)y * sp) * Wp + (int64_t)x * sp;
  for (int i = lane; i < sp * sp; i += kWave)
    dst[(int64_t)(i / sp) * Wp + (i % sp)] = i == win ? r : 0.f;
}

inline bool scale_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8 || s == 16; }

// rows of a (BN, Hp, Wp) map at scale sp, or -1 when the shape is not supported
inline int64_t row_count(int BN, int Hp, int Wp, int sp) {
  if (BN <= 0 || Hp <= 0 || Wp <= 0 || !scale_ok(sp) || Hp % sp || Wp % sp) return -1;
  const int64_t rows = (int64_t)BN * (Hp / sp) * (Wp / sp);
  // one workgroup per 4 rows in a 1-D grid
  return rows <= 0x7fffffffLL ? rows : -1;
}
}  // namespace

extern "C" {

int veon_depth_loss_rows(int BN, int Hp, int Wp, int sp, int Hg, int Wg, int sg, int D,
                         float lo, float step, float gamma, const float* depth,
                         const float* gt_depth, float* rec, void* stream) {
  const int64_t rows = row_count(BN, Hp, Wp, sp);
  if (rows < 0 || rows != row_count(BN, Hg, Wg, sg) || Hp / sp != Hg / sg ||
      Wp / sp != Wg / sg || D <= 0 || D > 0x7fff || !(step > 0.f) || !(gamma > 0.f) ||
      !depth || !gt_depth || !rec || (reinterpret_cast<uintptr_t>(rec) & 15u))
    return VEON_ERR_BAD_ARG;
  // bin centres as torch forms them (veon_two_hot_depth)
  const float off = (float)((double)lo + (double)step / 2.0);
  hipLaunchKernelGGL(k_depth_loss_rows,
                     dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)),
                     dim3(kRowBlock), 0, static_cast<hipStream_t>(stream), depth, gt_depth,
                     rows, Hp / sp, Wp / sp, sp, sg, D, step, off, gamma, rec);
  return launch_status();
}

int veon_depth_loss_reduce(int64_t rows, const float* rec, float* out, float* coef,
                           void* stream) {
  if (rows <= 0 || rows > 0x7fffffffLL || !rec || !out || !coef ||
      (reinterpret_cast<uintptr_t>(rec) & 15u))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_depth_loss_reduce, dim3(1), dim3(kReduceBlock), 0,
                     static_cast<hipStream_t>(stream), rec, rows, out, coef);
  return launch_status();
}

int veon_depth_loss_bwd(int BN, int Hp, int Wp, int sp, const float* rec, const float* coef,
                        const float* g_zoe, const float* g_ce, float* grad, void* stream) {
  const int64_t rows = row_count(BN, Hp, Wp, sp);
  if (rows < 0 || !rec || !coef || !grad || (reinterpret_cast<uintptr_t>(rec) & 15u))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_depth_loss_bwd,
                     dim3((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)),
                     dim3(kRowBlock), 0, static_cast<hipStream_t>(stream), rec, coef, g_zoe,
                     g_ce, rows, Hp / sp, Wp / sp, sp, grad);
  return launch_status();
}

}  // extern "C"
