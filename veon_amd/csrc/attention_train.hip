// Attention for training (head dim 64, with or without a dense additive bias): the forward
// that also records the softmax statistics, and the backward.
//
//   k_attention<false, false, true>   attention_kernel.h: the inference kernel with the
//                     score scale as an argument and lse[b][h][q] written next to out
//   k_attention<true, false, true>    the same with the fp32 bias added to the scaled scores
//   k_attention_delta delta[b][h][q] = sum_d dO[q][d] * O[q][d], fp32 (the unbiased pair)
//   k_attention_bwd<false>   dQ: a wave owns 32 queries, K / V tiles stream through LDS
//   k_attention_bwd<true>    dK and dV: a wave owns 32 keys, Q / dO tiles stream
//
// The two backward kernels are ONE body.  Call the rows a wave owns "own" (fragments in
// registers, B operands) and the rows of the 64-row LDS tiles "streamed" (A operands):
//
//                      own x   own y   streamed X   streamed Y
//   dQ  (DKV false)    Q       dO      K            V
//   dKV (DKV true)     K       V       Q            dO
//
//   s  = X . x^T     the raw scores: S^T (dQ) or S (dKV), 4 streamed rows x 1 own row
//   dp = Y . y^T     dP^T or dP                                            per lane
//   p  = exp2(s * scale * log2(e) - lse[query]),  ds = p * (dp - delta[query])
//   dQ :  dQ^T += K^T ds                       (transposing read on the X tile)
//   dKV:  dK^T += Q^T ds,  dV^T += dO^T p      (transposing reads on the X and Y tiles)
//
// The statistics are known, so there is no running maximum and no rescale.  In the dQ
// kernel the query is the lane's own row (two scalars per 16-query tile, loaded once);
// in the dKV kernel it is the streamed row (one aligned float4 of lse and of delta per
// 16-query tile).  Streamed rows >= T are clamped on load and their p and ds are set
// to zero BY INDEX, so columns T.. of lse / delta are never used.  Own rows >= T are
// clamped on load too and never stored; a column of an MFMA result depends on that
// column of the B operand alone, so they touch nothing else.
// Layouts, DMA map, swizzle and fragment reads are those of k_attention.
//
// HAS_BIAS (the CLIP tail): p = exp2(s * scale * log2(e) + bias[query][key] * log2(e) - lse),
// the bias addressed as in k_attention (``border``: token 0 has bias 0 by index; loads are
// clamped like the rows).  The dQ kernel visits every (query, key) pair exactly once and
// stores ds to dbias[b][h][query - border][key - border] (dense, no scale factor, skipped
// when dbias is NULL).  A masked key (bias -inf) has p = ds = 0; a query whose keys are all
// masked has lse = +inf, so its whole row of p and ds is exp2(-inf) = 0.
// MODE (dQ kernel with a bias only):
//   kBwdFull    as above
//   kBwdDsOnly  nothing upstream of qkv needs a gradient: the dQ accumulation and its stores
//               are left out and the pass only writes dbias
//   kBwdDelta   the biased pair's delta pass: delta[b][h][q] = sum_k p dp / sum_k p, fp32
//               from the unrounded p and dp, written to the workspace for the two passes
//               after it.  (The division by the sum of the REBUILT p, 1 within the 1e-6 of
//               the fp32 exponent and the hardware exp2 / log2, makes sum_k dS = 0 hold
//               for the p the passes use, as softmax's own backward has it; a fully masked
//               query has delta 0.)
//               k_attention_delta's dO . O carries the half rounding of O, u |dO . O|; on
//               the saturated rows a Gram-shaped bias makes (p of the own key within 1e-4
//               of 1) that is several times the row's whole dS, which p (dp - sum p dp)
//               gets right because the large own-key term cancels exactly (measured at
//               (2, 33, 2) in bf16: dq 1.5e-2 from dO . O, 2.2e-3 from sum p dp, against
//               2.9e-3 of torch's half arithmetic).
#include "attention_kernel.h"

namespace {

__global__ __launch_bounds__(256) void k_attention_delta(
    const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
    float* __restrict__ delta, int T, int H, int Tp, int64_t rows) {
  // 16 lanes per (b, q, h) row of 64 values: one 8-byte load of each tensor per lane
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int part = threadIdx.x & 15;
  float acc = 0.f;
  if (r < rows) {
    const uint2 a = *reinterpret_cast<const uint2*>(out + r * HD + part * 4);
    const uint2 g = *reinterpret_cast<const uint2*>(dout + r * HD + part * 4);
    acc = bf2f((bf16_t)(a.x & 0xffffu)) * bf2f((bf16_t)(g.x & 0xffffu));
    acc = fmaf(bf2f((bf16_t)(a.x >> 16)), bf2f((bf16_t)(g.x >> 16)), acc);
    acc = fmaf(bf2f((bf16_t)(a.y & 0xffffu)), bf2f((bf16_t)(g.y & 0xffffu)), acc);
    acc = fmaf(bf2f((bf16_t)(a.y >> 16)), bf2f((bf16_t)(g.y >> 16)), acc);
  }
  // (16-lane groups by shuffle width: no shared helper has this form)
#pragma unroll
  for (int m = 8; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 16);
  if (r < rows && part == 0) {
    const int h = (int)(r % H);
    const int64_t bt = r / H;
    const int q = (int)(bt % T);
    const int64_t b = bt / T;
    delta[(b * H + h) * Tp + q] = acc;
  }
}

constexpr float kLog2eF = 1.4426950408889634f;
enum { kBwdFull = 0, kBwdDsOnly = 1, kBwdDelta = 2 };

template <bool DKV, bool HAS_BIAS = false, int MODE = kBwdFull>
__global__ __launch_bounds__(256, 2) void k_attention_bwd(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16_t* __restrict__ dqkv, int T, int H, int Tp, float c_scale, float scale,
    const float* __restrict__ bias, int64_t bias_sb, int64_t bias_sh, int border,
    float* __restrict__ dbias, float* __restrict__ delta_out) {
  static_assert(MODE == kBwdFull || (HAS_BIAS && !DKV), "modes of the biased dQ kernel");
  constexpr bool GRAD = MODE == kBwdFull, DELTA = MODE == kBwdDelta;
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * KV_ELEMS];  // [buf][X|Y]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int r0 = (blockIdx.x * 4 + wave) * AQ;   // the wave's first own row
  const int tok_stride = 3 * H * HD, o_stride = H * HD;
  const bf16_t* qb = qkv + (int64_t)b * T * tok_stride + (int64_t)h * HD;
  const bf16_t* dob = dout + (int64_t)b * T * o_stride + (int64_t)h * HD;
  const float* lrow = lse + ((int64_t)b * H + h) * Tp;
  const float* drow = delta + ((int64_t)b * H + h) * Tp;
  // streamed (X, Y) and own (x, y) rows: base and row stride in elements
  const bf16_t* gX = DKV ? qb : qb + H * HD;
  const bf16_t* gY = DKV ? dob : qb + 2 * H * HD;
  const int strY = DKV ? o_stride : tok_stride;
  const bf16_t* gx = DKV ? qb + H * HD : qb;
  const bf16_t* gy = DKV ? qb + 2 * H * HD : dob;
  const int stry = DKV ? tok_stride : o_stride;

  int dr[2], dc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    dr[j] = (wave * 2 + j) * 8 + (lane >> 3);
    dc[j] = ((lane & 7) ^ (dr[j] & 7)) * 8;
  }
  const rsrc_t rsX = make_rsrc(gX), rsY = make_rsrc(gY);
  auto dma = [&](int buf, int k0) {
    bf16_t* dX = smem + buf * 2 * KV_ELEMS;
    bf16_t* dY = dX + KV_ELEMS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = k0 + dr[j] < T ? k0 + dr[j] : T - 1;
      const int slot = (wave * 2 + j) * 512;
      // byte offsets inside this image's rows (the launcher checks < 2^31)
      buffer_load_lds16(rsX, (lptr_t)(dX + slot), 2 * (row * tok_stride + dc[j]), 0);
      buffer_load_lds16(rsY, (lptr_t)(dY + slot), 2 * (row * strY + dc[j]), 0);
    }
  };
  dma(0, 0);

  // own fragments (B operands): lane holds x[row = fr][d = 32 ks + 8fg + j]
  bf16x8 xf[QT][2], yf[QT][2];
  float lse_o[QT], del_o[QT], psum[QT];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int r = r0 + i * 16 + fr;
    const int rc = r < T ? r : T - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      xf[i][ks] = *reinterpret_cast<const bf16x8*>(gx + (int64_t)rc * tok_stride + ks * 32 +
                                                   fg * 8);
      yf[i][ks] = *reinterpret_cast<const bf16x8*>(gy + (int64_t)rc * stry + ks * 32 +
                                                   fg * 8);
    }
    if (!DKV) {
      lse_o[i] = lrow[rc];
      del_o[i] = DELTA ? 0.f : drow[rc];   // (the delta pass: the running sum p dp)
      psum[i] = 0.f;
    }
  }
  // bias: own index (row of the matrix in the dQ kernel, column in the dKV kernel), clamped
  // into [0, Tb); own_b: the own token is not the bordered class token
  const int Tb = T - border;
  const float* bmat = nullptr;
  int own_i[QT];
  bool own_b[QT];
  if (HAS_BIAS) {
    bmat = bias + b * bias_sb + h * bias_sh;
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      const int r = r0 + i * 16 + fr;
      const int ro = (r < T ? r : T - 1) - border;
      own_b[i] = ro >= 0;
      own_i[i] = ro < 0 ? 0 : ro;
    }
  }
  // accumulators, transposed: acc[i][jt][reg] = grad[own row i*16 + fr][d = jt*16 + 4fg + reg]
  f32x4 accA[QT][4];   // dQ (dQ kernel) or dK (dKV kernel)
  f32x4 accV[QT][4];   // dV (dKV kernel only)
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      accA[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      accV[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  const int offK = fr * HD + ((fg ^ (fr & 7)) * 8);
  int offV[4];
  {
    const int row = 4 * fg + (fr >> 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int chunk = 2 * j + ((fr & 3) >> 1);
      offV[j] = row * HD + ((chunk ^ (row & 7)) * 8) + 4 * (fr & 1);
    }
  }

  const int nt = (T + AK - 1) / AK;
  auto tile = [&](int t, auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int k0 = t * AK;
    const bf16_t* sX = smem + (t & 1) * 2 * KV_ELEMS;
    const bf16_t* sY = sX + KV_ELEMS;
    // s[i][kt][reg], dp[i][kt][reg]: streamed row kt*16 + 4fg + reg, own row i*16 + fr
    f32x4 s[QT][4], dp[QT][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 X0 = *reinterpret_cast<const bf16x8*>(sX + kt * 16 * HD + offK);
      const bf16x8 X1 = *reinterpret_cast<const bf16x8*>(sX + kt * 16 * HD + (offK ^ 32));
      const bf16x8 Y0 = *reinterpret_cast<const bf16x8*>(sY + kt * 16 * HD + offK);
      const bf16x8 Y1 = *reinterpret_cast<const bf16x8*>(sY + kt * 16 * HD + (offK ^ 32));
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        f32x4 a = mfma_16x16x32(X0, xf[i][0], f32x4{0.f, 0.f, 0.f, 0.f});
        s[i][kt] = mfma_16x16x32(X1, xf[i][1], a);
        f32x4 g = mfma_16x16x32(Y0, yf[i][0], f32x4{0.f, 0.f, 0.f, 0.f});
        dp[i][kt] = mfma_16x16x32(Y1, yf[i][1], g);
      }
    }
    // p into s, ds into dp
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      f32x4 L4, D4;
      if (DKV) {
        L4 = *reinterpret_cast<const f32x4*>(lrow + k0 + kt * 16 + 4 * fg);
        D4 = *reinterpret_cast<const f32x4*>(drow + k0 + kt * 16 + 4 * fg);
      }
#pragma unroll
      for (int i = 0; i < QT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float l = DKV ? L4[r] : lse_o[i];
          const float dl = DKV ? D4[r] : del_o[i];
          float e = fmaf(s[i][kt][r], c_scale, -l);
          if (HAS_BIAS) {
            int ks = k0 + kt * 16 + 4 * fg + r;
            if (TAIL) ks = ks < T ? ks : T - 1;
            ks -= border;
            float bv = 0.f;
            if (own_b[i] && ks >= 0)
              bv = DKV ? bmat[(int64_t)ks * Tb + own_i[i]] : bmat[(int64_t)own_i[i] * Tb + ks];
            e = fmaf(bv, kLog2eF, e);
          }
          float p = __builtin_amdgcn_exp2f(e);
          float ds = p * (dp[i][kt][r] - dl);
          if (TAIL && k0 + kt * 16 + 4 * fg + r >= T) {
            p = 0.f;
            ds = 0.f;
          }
          if (DELTA) {
            del_o[i] = fmaf(p, dp[i][kt][r], del_o[i]);
            psum[i] += p;
          }
          s[i][kt][r] = p;
          dp[i][kt][r] = ds;
        }
    }
    if (DELTA) return;
    if (HAS_BIAS && !DKV && dbias != nullptr) {
      // every (query, key) pair of the matrix once: 16 bytes per lane and key tile
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const int q = r0 + i * 16 + fr;
        if (q >= T || q < border) continue;
        float* drow_b = dbias + (((int64_t)b * H + h) * Tb + (q - border)) * Tb;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + kt * 16 + 4 * fg + r;
            if ((!TAIL || key < T) && key >= border) drow_b[key - border] = dp[i][kt][r];
          }
      }
    }
    if (!GRAD) return;
    // acc^T += X^T ds (and Y^T p): MFMA k-slot (8fg + j) <-> streamed row
    //   j < 4 : row tile 2*kk,   rows 4fg + j
    //   j >= 4: row tile 2*kk+1, rows 4fg + (j-4)
    typedef unsigned __attribute__((ext_vector_type(4))) u32x4;
    auto pack8 = [](const f32x4& lo, const f32x4& hi) {
      const u32x4 pk = {pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]),
                        pack_bf16(hi[0], hi[1]), pack_bf16(hi[2], hi[3])};
      return __builtin_bit_cast(bf16x8, pk);
    };
    auto read_t = [&](const bf16_t* tile_base, int kk, int j) {
      const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(tile_base + (2 * kk) * 16 * HD + offV[j]));
      const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_bf16x4*)(tile_base + (2 * kk + 1) * 16 * HD + offV[j]));
      bf16x8 vf;
      vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
      vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
      return vf;
    };
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 pf[QT], dsf[QT];
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        dsf[i] = pack8(dp[i][2 * kk], dp[i][2 * kk + 1]);
        if (DKV) pf[i] = pack8(s[i][2 * kk], s[i][2 * kk + 1]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 xt = read_t(sX, kk, j);
#pragma unroll
        for (int i = 0; i < QT; ++i) accA[i][j] = mfma_16x16x32(xt, dsf[i], accA[i][j]);
        if (DKV) {
          const bf16x8 yt = read_t(sY, kk, j);
#pragma unroll
          for (int i = 0; i < QT; ++i) accV[i][j] = mfma_16x16x32(yt, pf[i], accV[i][j]);
        }
      }
    }
  };

  __syncthreads();  // tile 0 landed
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) dma((t + 1) & 1, (t + 1) * AK);  // flies under this tile
    if (r0 < T) {  // waves past the last row only feed the DMA and barriers
      if ((t + 1) * AK > T)
        tile(t, std::true_type{});
      else
        tile(t, std::false_type{});
    }
    __syncthreads();  // next tile landed, this one fully consumed
  }
  if (DELTA) {
    // the four lane rows of a query hold 16 keys of every tile each: added in a fixed order
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      float d = del_o[i], l = psum[i];
      // (16 then 32, low to high: written out, a helper changed the code)
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      l += __shfl_xor(l, 16);
      l += __shfl_xor(l, 32);
      const int r = r0 + i * 16 + fr;
      if (r < T && fg == 0) delta_out[((int64_t)b * H + h) * Tp + r] = l > 0.f ? d / l : 0.f;
    }
  }
  if (!GRAD) return;
  // store: lane owns grad[row = fr][d = j*16 + 4fg .. +3]; q and k thirds times scale
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int r = r0 + i * 16 + fr;
    if (r >= T) continue;
    bf16_t* dst = dqkv + ((int64_t)b * T + r) * tok_stride + (int64_t)h * HD +
                  (DKV ? H * HD : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint2 w2 = {pack_bf16(accA[i][j][0] * scale, accA[i][j][1] * scale),
                        pack_bf16(accA[i][j][2] * scale, accA[i][j][3] * scale)};
      *reinterpret_cast<uint2*>(dst + j * 16 + fg * 4) = w2;
      if (DKV) {
        const uint2 v2 = {pack_bf16(accV[i][j][0], accV[i][j][1]),
                          pack_bf16(accV[i][j][2], accV[i][j][3])};
        *reinterpret_cast<uint2*>(dst + H * HD + j * 16 + fg * 4) = v2;
      }
    }
  }
}

bool att_shape_ok(int B, int T, int H, int head_dim) {
  // the tile DMA addresses an image's rows with 32-bit byte offsets
  return B > 0 && T > 0 && H > 0 && head_dim == HD &&
         (int64_t)T * 3 * H * HD * 2 < (1ll << 31) && B <= 65535 && H <= 65535;
}

// the bias of the biased pair: fp32 [.][.][Tb][Tb], Tb = T - border, strides >= 0; with
// Tb == 0 (T = 1, border = 1) it is never read and may be NULL
bool bias_ok(const float* bias, int64_t sb, int64_t sh, int border, int T) {
  if (border != 0 && border != 1) return false;
  if (sb < 0 || sh < 0) return false;
  if (T - border == 0) return true;
  return bias != nullptr && (uintptr_t)bias % 4 == 0;
}

}  // namespace

extern "C" {

int64_t veon_vit_attention_stats_len(int T) {
  return T <= 0 ? 0 : ((int64_t)T + AK - 1) / AK * AK;
}

int veon_vit_attention_fwd_lse(const void* qkv, void* out, float* lse, int B, int T, int H,
                               int head_dim, float scale, void* stream) {
  if (!qkv || !out || !lse || !att_shape_ok(B, T, H, head_dim) || !(scale > 0.f))
    return VEON_ERR_BAD_ARG;
  if (!al16(qkv) || !al16(out) || !al16(lse)) return VEON_ERR_BAD_ARG;
  const dim3 grid((unsigned)((T + 4 * AQ - 1) / (4 * AQ)), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL((k_attention<false, false, true>), grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<const float*>(nullptr), (int64_t)0, (int64_t)0, 0,
                     static_cast<bf16_t*>(out), T, H, scale * kLog2eF, lse,
                     (int)veon_vit_attention_stats_len(T));
  return launch_status();
}

int64_t veon_vit_attention_bwd_workspace_bytes(int B, int T, int H) {
  if (B <= 0 || T <= 0 || H <= 0) return -1;
  return (int64_t)B * H * veon_vit_attention_stats_len(T) * (int64_t)sizeof(float);
}

int veon_vit_attention_bwd(const void* qkv, const void* out, const void* dout,
                           const float* lse, void* dqkv, void* workspace,
                           int64_t workspace_bytes, int B, int T, int H, int head_dim,
                           float scale, void* stream) {
  if (!qkv || !out || !dout || !lse || !dqkv || !workspace ||
      !att_shape_ok(B, T, H, head_dim) || !(scale > 0.f) || dqkv == qkv || dqkv == out ||
      dqkv == dout)
    return VEON_ERR_BAD_ARG;
  if (!al16(qkv) || !al16(out) || !al16(dout) || !al16(lse) || !al16(dqkv) ||
      !al16(workspace))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_vit_attention_bwd_workspace_bytes(B, T, H))
    return VEON_ERR_WORKSPACE;
  const int Tp = (int)veon_vit_attention_stats_len(T);
  const int64_t rows = (int64_t)B * T * H;
  const int64_t dblocks = (rows * 16 + 255) / 256;
  if (dblocks > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* delta = static_cast<float*>(workspace);
  const bf16_t* q = static_cast<const bf16_t*>(qkv);
  const bf16_t* go = static_cast<const bf16_t*>(dout);
  hipLaunchKernelGGL(k_attention_delta, dim3((unsigned)dblocks), dim3(256), 0, s,
                     static_cast<const bf16_t*>(out), go, delta, T, H, Tp, rows);
  const dim3 grid((unsigned)((T + 4 * AQ - 1) / (4 * AQ)), (unsigned)H, (unsigned)B);
  const float c = scale * kLog2eF;
  hipLaunchKernelGGL((k_attention_bwd<false>), grid, dim3(256), 0, s, q, go, lse, delta,
                     static_cast<bf16_t*>(dqkv), T, H, Tp, c, scale,
                     static_cast<const float*>(nullptr), (int64_t)0, (int64_t)0, 0,
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  hipLaunchKernelGGL((k_attention_bwd<true>), grid, dim3(256), 0, s, q, go, lse, delta,
                     static_cast<bf16_t*>(dqkv), T, H, Tp, c, scale,
                     static_cast<const float*>(nullptr), (int64_t)0, (int64_t)0, 0,
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  return launch_status();
}

int veon_vit_attention_bias_fwd_lse(const void* qkv, const float* bias, int64_t bias_sb,
                                    int64_t bias_sh, int border, void* out, float* lse, int B,
                                    int T, int H, int head_dim, float scale, void* stream) {
  if (!qkv || !out || !lse || !att_shape_ok(B, T, H, head_dim) || !(scale > 0.f) ||
      !bias_ok(bias, bias_sb, bias_sh, border, T))
    return VEON_ERR_BAD_ARG;
  if (!al16(qkv) || !al16(out) || !al16(lse)) return VEON_ERR_BAD_ARG;
  const dim3 grid((unsigned)((T + 4 * AQ - 1) / (4 * AQ)), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL((k_attention<true, false, true>), grid, dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv), bias,
                     bias_sb, bias_sh, border, static_cast<bf16_t*>(out), T, H,
                     scale * kLog2eF, lse, (int)veon_vit_attention_stats_len(T));
  return launch_status();
}

int veon_vit_attention_bias_bwd(const void* qkv, const float* bias, int64_t bias_sb,
                                int64_t bias_sh, int border, const void* out, const void* dout,
                                const float* lse, void* dqkv, float* dbias, void* workspace,
                                int64_t workspace_bytes, int B, int T, int H, int head_dim,
                                float scale, void* stream) {
  if (!qkv || !out || !dout || !lse || (!dqkv && !dbias) || !workspace ||
      !att_shape_ok(B, T, H, head_dim) || !(scale > 0.f) ||
      !bias_ok(bias, bias_sb, bias_sh, border, T))
    return VEON_ERR_BAD_ARG;
  if (dqkv && (dqkv == qkv || dqkv == out || dqkv == dout || !al16(dqkv)))
    return VEON_ERR_BAD_ARG;
  if (dbias && ((uintptr_t)dbias % 4 != 0 || dbias == bias)) return VEON_ERR_BAD_ARG;
  if (!al16(qkv) || !al16(out) || !al16(dout) || !al16(lse) || !al16(workspace))
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_vit_attention_bwd_workspace_bytes(B, T, H))
    return VEON_ERR_WORKSPACE;
  const int Tp = (int)veon_vit_attention_stats_len(T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* delta = static_cast<float*>(workspace);
  const bf16_t* q = static_cast<const bf16_t*>(qkv);
  const bf16_t* go = static_cast<const bf16_t*>(dout);
  bf16_t* dq = static_cast<bf16_t*>(dqkv);
  const dim3 grid((unsigned)((T + 4 * AQ - 1) / (4 * AQ)), (unsigned)H, (unsigned)B);
  const float c = scale * kLog2eF;
  float* none = nullptr;
  // delta = sum_k p dp from the probabilities themselves (see kBwdDelta above)
  hipLaunchKernelGGL((k_attention_bwd<false, true, kBwdDelta>), grid, dim3(256), 0, s, q, go,
                     lse, delta, dq, T, H, Tp, c, scale, bias, bias_sb, bias_sh, border, none,
                     delta);
  if (dq) {
    hipLaunchKernelGGL((k_attention_bwd<false, true, kBwdFull>), grid, dim3(256), 0, s, q, go,
                       lse, delta, dq, T, H, Tp, c, scale, bias, bias_sb, bias_sh, border,
                       dbias, none);
    hipLaunchKernelGGL((k_attention_bwd<true, true, kBwdFull>), grid, dim3(256), 0, s, q, go,
                       lse, delta, dq, T, H, Tp, c, scale, bias, bias_sb, bias_sh, border, none,
                       none);
  } else {
    hipLaunchKernelGGL((k_attention_bwd<false, true, kBwdDsOnly>), grid, dim3(256), 0, s, q,
                       go, lse, delta, dq, T, H, Tp, c, scale, bias, bias_sb, bias_sh, border,
                       dbias, none);
  }
  return launch_status();
}

}  // extern "C"
