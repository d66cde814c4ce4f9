// Backward of k_deform_attn (csrc/temporal.hip), the sampling + attention core of
// TemporalDeformable (mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:138-196),
// on the same padded channels-last half grids.  Nothing of the forward is stored but its
// inputs: every sample position is recomputed by deform_pos.h, bit for bit.
//
// Per voxel v, head h, sample s, in fp32 (K_s, V_s: trilinear samples of the head's
// [key | value] rows; scale = hd^-0.5):
//   a = softmax_s(scale q.K_s)          da_s = dOut.V_s
//   dl_s = a_s (da_s - sum_t a_t da_t)  dq = scale sum_s dl_s K_s
//   g_s = [scale dl_s q | a_s dOut]     dKV[row of corner c] += w_{s,c} g_s
//   d f_axis = sum_c (+-1) (product of the other two axes' weights) (row_c . g_s)
//   dOff = d f_axis * 0.5 (n_dst - 1) / n_src * (1 - tanh^2(o)), zero where f <= 0 or
//   f >= n_dst - 1 (ATen's border convention; covers the clamp and axes of length one)
//
//  * k_deform_attn_bwd: the forward's lane layout, one voxel per lane group.  Writes dq,
//    dOff and one fp32 record (scale dl_s, a_s) per (voxel, head, sample).
//  * k_deform_attn_bwd_dkv: one lane group per TARGET row of dKV, a gather over the box of
//    source voxels that can reach it (three (lo, hi) tables from the host): no atomics,
//    a fixed order, every row written (halo and unreached rows get zeros).
#include <hip/hip_runtime.h>

#include "deform_pos.h"
#include "mfma_common.h"
#include "veon_hip.h"

namespace {

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

template <int HD>
__global__ __launch_bounds__(256) void k_deform_attn_bwd(
    const bf16_t* __restrict__ kv, const bf16_t* __restrict__ q,
    const bf16_t* __restrict__ off, const bf16_t* __restrict__ dout,
    bf16_t* __restrict__ dq, bf16_t* __restrict__ doff, float2* __restrict__ rec, int B,
    int Z, int Y, int X, int heads, int off_stride, float qscale) {
  constexpr int KL = HD / 8;       // key lanes (= value lanes) per head
  constexpr int LPH = 2 * KL;
  constexpr int S = kDeformSamples;
  const int lpv = heads * LPH;     // lanes per voxel, divides 64 (host-checked)
  const int vpw = 64 / lpv;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t nvox = (int64_t)B * Z * Y * X;
  int64_t v = ((int64_t)blockIdx.x * 4 + wave) * vpw + lane / lpv;
  const bool live = v < nvox;
  if (!live) v = nvox - 1;         // keep the lane in the shuffles
  const int r = lane % lpv;
  const int h = r / LPH;
  const int j = r % LPH;
  const bool is_val = j >= KL;
  const int x = (int)(v % X);
  const int y = (int)((v / X) % Y);
  const int z = (int)((v / ((int64_t)X * Y)) % Z);
  const int b = (int)(v / ((int64_t)X * Y * Z));
  const int Yp = Y + 2, Xp = X + 2;
  const int64_t plane0 = (int64_t)b * (Z + 2);
  const int64_t row = ((plane0 + z + 1) * Yp + y + 1) * Xp + x + 1;
  const int C = heads * HD;

  // key lanes: 8 query channels (scaled as in the forward); value lanes: 8 of dOut
  float u[8];
  {
    const bf16x8 t = ld8((is_val ? dout : q) + row * C + h * HD + (j & (KL - 1)) * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = is_val ? bf2f((bf16_t)t[k]) : bf2f((bf16_t)t[k]) * qscale;
  }
  const float zn = deform_base(z, Z), yn = deform_base(y, Y), xn = deform_base(x, X);
  const bf16_t* orow = off + row * off_stride + h * S * 3;
  const bf16_t* kvh = kv + h * 2 * HD + j * 8;
  const int64_t kvc = 2 * C;
  // d f / d raw offset without the (1 - tanh^2) factor
  const float jx = 0.5f * (X - 1) / Z, jy = 0.5f * (Y - 1) / Y, jz = 0.5f * (Z - 1) / X;

  float samp[S][8];            // K_s (key lanes) / V_s (value lanes)
  float logit[S], da[S];
  float pk[S][3], pv[S][3];    // position gradients of the logit / of da, times d f / d o
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const DeformPos p = deform_pos(orow + s * 3, zn, yn, xn, Z, Y, X);
#pragma unroll
    for (int k = 0; k < 8; ++k) samp[s][k] = 0.f;
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int zc = (c & 4) ? p.z1 : p.z0, yc = (c & 2) ? p.y1 : p.y0,
                xc = (c & 1) ? p.x1 : p.x0;
      const float wz = (c & 4) ? p.tz : 1.f - p.tz, wy = (c & 2) ? p.ty : 1.f - p.ty,
                  wx = (c & 1) ? p.tx : 1.f - p.tx;
      const int64_t rr = ((plane0 + zc + 1) * Yp + yc + 1) * Xp + xc + 1;
      const bf16x8 t = ld8(kvh + rr * kvc);
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float e = bf2f((bf16_t)t[k]);
        samp[s][k] = fmaf(wz * wy * wx, e, samp[s][k]);
        d = fmaf(u[k], e, d);
      }
      gx += (c & 1) ? wz * wy * d : -(wz * wy * d);
      gy += (c & 2) ? wz * wx * d : -(wz * wx * d);
      gz += (c & 4) ? wy * wx * d : -(wy * wx * d);
    }
    float part = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) part = fmaf(u[k], samp[s][k], part);
    // ATen: no gradient through a coordinate on or beyond the border
    gx = (p.fx > 0.f && p.fx < (float)(X - 1)) ? gx * jx * (1.f - p.o0 * p.o0) : 0.f;
    gy = (p.fy > 0.f && p.fy < (float)(Y - 1)) ? gy * jy * (1.f - p.o1 * p.o1) : 0.f;
    gz = (p.fz > 0.f && p.fz < (float)(Z - 1)) ? gz * jz * (1.f - p.o2 * p.o2) : 0.f;
    // (KL-split sums of four values in step, 1 up to KL / 2: written out)
#pragma unroll
    for (int d = 1; d < KL; d <<= 1) {
      part += __shfl_xor(part, d);
      gx += __shfl_xor(gx, d);
      gy += __shfl_xor(gy, d);
      gz += __shfl_xor(gz, d);
    }
    const float opart = __shfl_xor(part, KL), ox = __shfl_xor(gx, KL),
                oy = __shfl_xor(gy, KL), oz = __shfl_xor(gz, KL);
    logit[s] = is_val ? opart : part;
    da[s] = is_val ? part : opart;
    pk[s][0] = is_val ? ox : gx;
    pk[s][1] = is_val ? oy : gy;
    pk[s][2] = is_val ? oz : gz;
    pv[s][0] = is_val ? gx : ox;
    pv[s][1] = is_val ? gy : oy;
    pv[s][2] = is_val ? gz : oz;
  }

  float m = logit[0];
#pragma unroll
  for (int s = 1; s < S; ++s) m = fmaxf(m, logit[s]);
  float a[S], l = 0.f;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a[s] = __expf(logit[s] - m);
    l += a[s];
  }
  const float inv = 1.f / l;
  float mean = 0.f;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    a[s] *= inv;
    mean = fmaf(a[s], da[s], mean);
  }
  float dl[S];
#pragma unroll
  for (int s = 0; s < S; ++s) dl[s] = a[s] * (da[s] - mean);

  if (!live) return;               // no shuffles below
  if (!is_val) {
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = 0.f;
#pragma unroll
      for (int s = 0; s < S; ++s) t = fmaf(dl[s], samp[s][k], t);
      o[k] = (short)f2bf(t * qscale);
    }
    *reinterpret_cast<bf16x8*>(dq + row * C + h * HD + j * 8) = o;
  }
  // every lane of the head holds all 8 samples' scalars: lane j stores what falls to it
  float2* vrec = rec + (v * heads + h) * S;
  bf16_t* drow = doff + row * off_stride;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (j == s) vrec[s] = make_float2(qscale * dl[s], a[s]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (j == (s * 3 + c) % LPH)
        drow[h * S * 3 + s * 3 + c] = f2bf(fmaf(dl[s], pk[s][c], a[s] * pv[s][c]));
  }
  for (int ch = heads * S * 3 + r; ch < off_stride; ch += lpv) drow[ch] = 0;   // surplus
}

// zero the halo rows of a padded grid of ANY channel count (2-byte stores)
__global__ __launch_bounds__(256) void k_zero_halo_any(bf16_t* __restrict__ rows, int planes,
                                                        int Zp, int Yp, int Xp, int C) {
  const int cpr = (C + 7) / 8;     // 8-channel chunks per row
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rrow = t / cpr;
  if (rrow >= (int64_t)planes * Yp * Xp) return;
  const int x = (int)(rrow % Xp);
  const int y = (int)((rrow / Xp) % Yp);
  const int z = (int)((rrow / ((int64_t)Xp * Yp)) % Zp);
  if (x == 0 || x == Xp - 1 || y == 0 || y == Yp - 1 || z == 0 || z == Zp - 1) {
    const int c0 = (int)(t % cpr) * 8;
    for (int c = c0; c < min(c0 + 8, C); ++c) rows[rrow * C + c] = 0;
  }
}

// One lane group (the forward's layout) per row of the padded dKV grid.  The source
// voxels that can touch target (zc, yc, xc) form a box: z in tabs_x[xc], y in tabs_y[yc],
// x in tabs_z[zc] (the axis quirk: the X position is driven by the z index).  Lane j of a
// head evaluates sample j & 7 of the source voxel; the weight of the lane group's own row,
// times the record, is summed over the 8 samples by a butterfly and multiplies the source
// voxel's q (key lanes) or dOut (value lanes) row.
template <int HD>
__global__ __launch_bounds__(256) void k_deform_attn_bwd_dkv(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ off,
    const bf16_t* __restrict__ dout, const float2* __restrict__ rec,
    const int* __restrict__ tabs, bf16_t* __restrict__ dkv, int B, int Z, int Y, int X,
    int heads, int off_stride) {
  constexpr int KL = HD / 8;
  constexpr int LPH = 2 * KL;
  constexpr int S = kDeformSamples;
  const int lpv = heads * LPH;
  const int vpw = 64 / lpv;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int Zp = Z + 2, Yp = Y + 2, Xp = X + 2;
  const int64_t nrows = (int64_t)B * Zp * Yp * Xp;
  int64_t t = ((int64_t)blockIdx.x * 4 + wave) * vpw + lane / lpv;
  const bool live = t < nrows;
  if (!live) t = nrows - 1;        // a halo row: empty box
  const int r = lane % lpv;
  const int h = r / LPH;
  const int j = r % LPH;
  const bool is_val = j >= KL;
  const int s = j & (S - 1);
  const int xc = (int)(t % Xp) - 1;
  const int yc = (int)((t / Xp) % Yp) - 1;
  const int zc = (int)((t / ((int64_t)Xp * Yp)) % Zp) - 1;
  const int b = (int)(t / ((int64_t)Xp * Yp * Zp));
  const int C = heads * HD;

  int zlo = 0, zhi = -1, ylo = 0, yhi = -1, xlo = 0, xhi = -1;
  if (xc >= 0 && xc < X && yc >= 0 && yc < Y && zc >= 0 && zc < Z) {
    const int* ty = tabs + 2 * X;
    const int* tz = ty + 2 * Y;
    zlo = max(tabs[2 * xc], 0), zhi = min(tabs[2 * xc + 1], Z - 1);
    ylo = max(ty[2 * yc], 0), yhi = min(ty[2 * yc + 1], Y - 1);
    xlo = max(tz[2 * zc], 0), xhi = min(tz[2 * zc + 1], X - 1);
  }
  const int n = max(zhi - zlo + 1, 0) * max(yhi - ylo + 1, 0) * max(xhi - xlo + 1, 0);
  int nmax = n;                    // the wave walks its longest box
  // (a max over a run-time lane stride: no shared helper)
  for (int d = lpv; d < 64; d <<= 1) nmax = max(nmax, __shfl_xor(nmax, d));

  const int64_t plane0 = (int64_t)b * Zp;
  const bf16_t* usrc = (is_val ? dout : q) + h * HD + (j & (KL - 1)) * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int iz = zlo, iy = ylo, ix = xlo;
  for (int i = 0; i < nmax; ++i) {
    const bool on = i < n;
    const int sz = on ? iz : 0, sy = on ? iy : 0, sx = on ? ix : 0;
    const int64_t srow = ((plane0 + sz + 1) * Yp + sy + 1) * Xp + sx + 1;
    const int64_t sv = (((int64_t)b * Z + sz) * Y + sy) * X + sx;
    const DeformPos p = deform_pos(off + srow * off_stride + (h * S + s) * 3,
                                   deform_base(sz, Z), deform_base(sy, Y),
                                   deform_base(sx, X), Z, Y, X);
    // weight of this row among the sample's corners; at the border both corners of an
    // axis are the same row
    const float wx = (p.x0 == xc ? 1.f - p.tx : 0.f) + (p.x1 == xc ? p.tx : 0.f);
    const float wy = (p.y0 == yc ? 1.f - p.ty : 0.f) + (p.y1 == yc ? p.ty : 0.f);
    const float wz = (p.z0 == zc ? 1.f - p.tz : 0.f) + (p.z1 == zc ? p.tz : 0.f);
    const float w = wz * wy * wx;
    const float2 rc = rec[(sv * heads + h) * S + s];
    float ck = on ? w * rc.x : 0.f, cv = on ? w * rc.y : 0.f;
    // (S-split sums of two values in step, 1 up to S / 2: written out)
#pragma unroll
    for (int d = 1; d < S; d <<= 1) {
      ck += __shfl_xor(ck, d);
      cv += __shfl_xor(cv, d);
    }
    const float coef = is_val ? cv : ck;
    const bf16x8 uu = ld8(usrc + srow * C);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = fmaf(coef, bf2f((bf16_t)uu[k]), acc[k]);
    if (on && ++ix > xhi) {
      ix = xlo;
      if (++iy > yhi) {
        iy = ylo;
        ++iz;
      }
    }
  }
  if (live) {
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (short)f2bf(acc[k]);
    *reinterpret_cast<bf16x8*>(dkv + t * (2 * C) + h * 2 * HD + j * 8) = o;
  }
}

// shape checks shared by the entry points; -> head dim, or 0
int deform_shape_ok(int B, int Z, int Y, int X, int C, int heads, int samples,
                    int off_channels) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || heads <= 0 || C <= 0 || C % heads != 0 ||
      samples != kDeformSamples || off_channels < heads * samples * 3)
    return 0;
  const int hd = C / heads;
  if (hd != 32 && hd != 64) return 0;
  const int lpv = heads * 2 * (hd / 8);
  if (lpv > 64 || 64 % lpv != 0) return 0;
  if ((int64_t)B * (Z + 2) * (Y + 2) * (X + 2) > 0x3fffffffLL) return 0;
  return hd;
}

}  // namespace

extern "C" {

int64_t veon_deform_attention_bwd_workspace_bytes(int B, int Z, int Y, int X, int heads) {
  if (B <= 0 || Z <= 0 || Y <= 0 || X <= 0 || heads <= 0) return -1;
  return (int64_t)B * Z * Y * X * heads * kDeformSamples * (int64_t)sizeof(float2);
}

int veon_deform_attention_bwd_bf16(const void* kv_padded, const void* q_padded,
                                   const void* off_padded, const void* dout_padded,
                                   void* dq_padded, void* doff_padded, void* workspace,
                                   int64_t workspace_bytes, int B, int Z, int Y, int X,
                                   int C, int heads, int samples, int off_channels,
                                   void* stream) {
  const int hd = deform_shape_ok(B, Z, Y, X, C, heads, samples, off_channels);
  if (!hd || !kv_padded || !q_padded || !off_padded || !dout_padded || !dq_padded ||
      !doff_padded || !workspace)
    return VEON_ERR_BAD_ARG;
  if (!al16(kv_padded) || !al16(q_padded) || !al16(dout_padded) || !al16(dq_padded) ||
      ((uintptr_t)off_padded & 1) || ((uintptr_t)doff_padded & 1) ||
      ((uintptr_t)workspace & 7))
    return VEON_ERR_BAD_ARG;
  if (dq_padded == q_padded || dq_padded == dout_padded || doff_padded == off_padded)
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_deform_attention_bwd_workspace_bytes(B, Z, Y, X, heads))
    return VEON_ERR_WORKSPACE;
  const int lpv = heads * 2 * (hd / 8);
  const int64_t nvox = (int64_t)B * Z * Y * X;
  const int vpb = 4 * (64 / lpv);  // voxels per 256-thread workgroup
  const int64_t blocks = (nvox + vpb - 1) / vpb;
  const int64_t prow = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  const int64_t hq = (prow * (C / 8) + 255) / 256;
  const int64_t ho = (prow * ((off_channels + 7) / 8) + 255) / 256;
  if (blocks > 0x7fffffffLL || hq > 0x7fffffffLL || ho > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float qscale = 1.f / sqrtf((float)hd);
  const bf16_t* KV = static_cast<const bf16_t*>(kv_padded);
  const bf16_t* Q = static_cast<const bf16_t*>(q_padded);
  const bf16_t* O = static_cast<const bf16_t*>(off_padded);
  const bf16_t* DO = static_cast<const bf16_t*>(dout_padded);
  bf16_t* dq = static_cast<bf16_t*>(dq_padded);
  bf16_t* doff = static_cast<bf16_t*>(doff_padded);
  float2* rec = static_cast<float2*>(workspace);
  hipLaunchKernelGGL(k_zero_halo_any, dim3((unsigned)hq), dim3(256), 0, s, dq, B * (Z + 2),
                     Z + 2, Y + 2, X + 2, C);
  hipLaunchKernelGGL(k_zero_halo_any, dim3((unsigned)ho), dim3(256), 0, s, doff, B * (Z + 2),
                     Z + 2, Y + 2, X + 2, off_channels);
  if (hd == 64)
    hipLaunchKernelGGL(k_deform_attn_bwd<64>, dim3((unsigned)blocks), dim3(256), 0, s, KV, Q,
                       O, DO, dq, doff, rec, B, Z, Y, X, heads, off_channels, qscale);
  else
    hipLaunchKernelGGL(k_deform_attn_bwd<32>, dim3((unsigned)blocks), dim3(256), 0, s, KV, Q,
                       O, DO, dq, doff, rec, B, Z, Y, X, heads, off_channels, qscale);
  return launch_status();
}

int veon_deform_attention_bwd_dkv_bf16(const void* q_padded, const void* off_padded,
                                       const void* dout_padded, const void* workspace,
                                       int64_t workspace_bytes, const int* ranges,
                                       void* dkv_padded, int B, int Z, int Y, int X, int C,
                                       int heads, int samples, int off_channels,
                                       void* stream) {
  const int hd = deform_shape_ok(B, Z, Y, X, C, heads, samples, off_channels);
  if (!hd || !q_padded || !off_padded || !dout_padded || !workspace || !ranges || !dkv_padded)
    return VEON_ERR_BAD_ARG;
  if (!al16(q_padded) || !al16(dout_padded) || !al16(dkv_padded) ||
      ((uintptr_t)off_padded & 1) || ((uintptr_t)workspace & 7) || ((uintptr_t)ranges & 3))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_deform_attention_bwd_workspace_bytes(B, Z, Y, X, heads))
    return VEON_ERR_WORKSPACE;
  const int lpv = heads * 2 * (hd / 8);
  const int64_t prow = (int64_t)B * (Z + 2) * (Y + 2) * (X + 2);
  const int rpb = 4 * (64 / lpv);  // target rows per 256-thread workgroup
  const int64_t blocks = (prow + rpb - 1) / rpb;
  if (blocks > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bf16_t* Q = static_cast<const bf16_t*>(q_padded);
  const bf16_t* O = static_cast<const bf16_t*>(off_padded);
  const bf16_t* DO = static_cast<const bf16_t*>(dout_padded);
  const float2* rec = static_cast<const float2*>(workspace);
  bf16_t* dkv = static_cast<bf16_t*>(dkv_padded);
  if (hd == 64)
    hipLaunchKernelGGL(k_deform_attn_bwd_dkv<64>, dim3((unsigned)blocks), dim3(256), 0, s, Q,
                       O, DO, rec, ranges, dkv, B, Z, Y, X, heads, off_channels);
  else
    hipLaunchKernelGGL(k_deform_attn_bwd_dkv<32>, dim3((unsigned)blocks), dim3(256), 0, s, Q,
                       O, DO, rec, ranges, dkv, B, Z, Y, X, heads, off_channels);
  return launch_status();
}

}  // extern "C"
