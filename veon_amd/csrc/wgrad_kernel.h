// The weight gradient of the 3x3 and 3x3x3 stride-1 pad-1 convolutions on padded
// channels-last half rows: ONE kernel body for conv3d_train.hip (27 taps, one (kz, ky)
// pair per workgroup) and conv2d_train.hip (9 taps, one ky per workgroup).  A tap is a
// constant row offset in both layouts, so the two differ only in how the workgroup's
// index becomes that offset and in the tap count of the output slab; the contraction
// and its accumulation order are the same code.  linear_train.hip instantiates the same
// body as the one-tap case with no row offset (NZY = 0): dW[N][K] = dy^T x of plain token
// rows, which have no guard rows -- that instantiation alone bounds its resources at the
// M rows and zeroes the tail of a partial last slab.  The host half (plan, dynamic-LDS
// size, launch, reduce) follows the kernels, templated on the same NZY.  Included inside
// each file's translation unit after mfma_common.h.
#pragma once
#include "mfma_common.h"

namespace {


typedef bf16x4 __attribute__((address_space(3))) lds_bf16x4;

constexpr int WBK = 64;   // rows of the contraction per LDS slab

// NZY = 9 / 3: three kx taps per workgroup, NZY workgroups per tile; NZY = 0: the linear
// layer, one tap and one workgroup per tile.
constexpr int wgrad_taps(int NZY) { return NZY == 0 ? 1 : 3; }
constexpr int wgrad_groups(int NZY) { return NZY == 0 ? 1 : NZY; }

// XOR key of the 16-byte chunks of an LDS row holding `chunks` (8 or 16) of them; for
// 256-byte rows the image of the programming guide's transposed-read section.  Applied
// on the DMA source address and again on the fragment read, per lane and per chunk.
__device__ __forceinline__ int tr_key(int row, int chunks) {
  return (((row & 3) << 2) | ((row >> 2) & 3)) & (chunks - 1);
}

// Dynamic LDS of k_conv_k3_wgrad<TI, TJ, *>: two buffers of [WBK rows of dy | rows
// k0 - 1 .. k0 + WBK of x (one tap: rows k0 .. k0 + WBK - 1), rounded up to whole 1 KiB
// DMA pieces].  The kernel asserts that this is what it addresses.
constexpr int wgrad_lds_bytes(int TI, int TJ, int NT) {
  const int rpx = 64 / (32 * TJ / 8);   // x rows per DMA piece
  return 2 * (WBK * 32 * TI + (WBK + NT - 1 + rpx - 1) / rpx * rpx * 32 * TJ) *
         (int)sizeof(bf16_t);
}

// Cout tile = 32 TI, Cin tile = 32 TJ; 2 x 2 waves of (16 TI) x (16 TJ) x 3 taps each.
// NZY = 9: 3-D grid, the workgroup's zy = 3 (dz + 1) + (dy + 1); NZY = 3: 2-D images
// (Yp is unused), zy = dy + 1.  The slab is [Cout][3 NZY][Cin].  NZY = 0: plain rows
// dy [M][Cout], x [M][Cin] (Yp, Xp unused; M is read by this case only), slab [Cout][Cin].
template <int TI, int TJ, int NZY>
__global__ __launch_bounds__(256) void k_conv_k3_wgrad(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* __restrict__ ws,
    int Yp, int Xp, int Cin, int Cout, int nsteps, int steps_per_split, int nco, int nci,
    int M) {
  constexpr int NT = wgrad_taps(NZY), NSLAB = NT * wgrad_groups(NZY);
  constexpr int CO_T = 32 * TI, CI_T = 32 * TJ;
  constexpr int CHD = CO_T / 8, CHX = CI_T / 8;      // 16-byte chunks per LDS row
  constexpr int RPD = 64 / CHD, RPX = 64 / CHX;      // rows per 1 KiB DMA piece
  constexpr int DPIECES = WBK / RPD;
  constexpr int XPIECES = (WBK + NT - 1 + RPX - 1) / RPX;  // rows k0 - 1 .. k0 + 64
  constexpr int D_ELEMS = WBK * CO_T, X_ELEMS = XPIECES * RPX * CI_T;
  constexpr int BUF_ELEMS = D_ELEMS + X_ELEMS;
  constexpr int DP = (DPIECES + 3) / 4, XP = (XPIECES + 3) / 4;
  static_assert(wgrad_lds_bytes(TI, TJ, NT) == 2 * BUF_ELEMS * (int)sizeof(bf16_t),
                "the launch allocates what the kernel addresses");
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];   // [2][dy | x]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wco = wave >> 1, wci = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;

  int t = blockIdx.x;
  const int ci_t = t % nci; t /= nci;
  const int co_t = t % nco;
  const int zy = t / nco;                     // 3 (dz + 1) + (dy + 1), or dy + 1
  const int split = blockIdx.y;
  const int s0 = split * steps_per_split;
  const int s1 = s0 + steps_per_split < nsteps ? s0 + steps_per_split : nsteps;

  // LDS row j of the x slab of step s holds padded row 64 s + j + offrow; tap dx reads
  // slab rows k + dx.  Rows outside [0, M) are guard rows (zeros).
  // One tap: no offset and no guard rows.  The resources end with row M - 1 of this
  // tile's columns, so a lane of a row >= M fails the range check and reads nothing.
  const int offrow = NZY == 0   ? 0
                     : NZY == 9 ? ((zy / 3 - 1) * Yp + (zy % 3 - 1)) * Xp - 1
                                : (zy - 1) * Xp - 1;
  const rsrc_t rsD = NZY == 0 ? make_rsrc_bounded(dy + co_t * CO_T,
                                                  2u * (unsigned)(M * Cout - co_t * CO_T))
                              : make_rsrc(dy + co_t * CO_T);
  const rsrc_t rsX = NZY == 0 ? make_rsrc_bounded(x + ci_t * CI_T,
                                                  2u * (unsigned)(M * Cin - ci_t * CI_T))
                              : make_rsrc(x + (int64_t)offrow * Cin + ci_t * CI_T);
  int srcD[DP], srcX[XP];
#pragma unroll
  for (int j = 0; j < DP; ++j) {
    const int r = (wave + 4 * j) * RPD + lane / CHD;
    const int c = (lane % CHD) ^ tr_key(r, CHD);
    srcD[j] = 2 * (r * Cout + c * 8);
  }
#pragma unroll
  for (int j = 0; j < XP; ++j) {
    const int r = (wave + 4 * j) * RPX + lane / CHX;
    const int c = (lane % CHX) ^ tr_key(r, CHX);
    srcX[j] = 2 * (r * Cin + c * 8);
  }
  auto dma = [&](int buf, int step) {
    bf16_t* dD = smem + buf * BUF_ELEMS;
    bf16_t* dX = dD + D_ELEMS;
    const int k0 = step * WBK;
    // The range check of a raw buffer compares the VECTOR offset with the record count and
    // leaves the scalar offset out: under a bounded resource the slab base rides in the
    // vector offset.
    const int vD = NZY == 0 ? 2 * k0 * Cout : 0, sD = NZY == 0 ? 0 : 2 * k0 * Cout;
    const int vX = NZY == 0 ? 2 * k0 * Cin : 0, sX = NZY == 0 ? 0 : 2 * k0 * Cin;
#pragma unroll
    for (int j = 0; j < DP; ++j)
      if (wave + 4 * j < DPIECES)   // wave-uniform
        buffer_load_lds16(rsD, (lptr_t)(dD + (wave + 4 * j) * 512), srcD[j] + vD, sD);
#pragma unroll
    for (int j = 0; j < XP; ++j)
      if (wave + 4 * j < XPIECES)
        buffer_load_lds16(rsX, (lptr_t)(dX + (wave + 4 * j) * 512), srcX[j] + vX, sX);
  };
  // Rows >= M of the (landed) last slab, both operands: zeros by plain LDS stores, so the
  // tail adds exactly 0 whatever a range-checked DMA lane left in its 16 bytes.
  auto zero_tail = [&](int buf, int first) {
    bf16_t* dD = smem + buf * BUF_ELEMS;
    bf16_t* dX = dD + D_ELEMS;
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = first * CHD + tid; i < WBK * CHD; i += 256)
      *reinterpret_cast<bf16x8*>(dD + i * 8) = z;
    for (int i = first * CHX + tid; i < WBK * CHX; i += 256)
      *reinterpret_cast<bf16x8*>(dX + i * 8) = z;
  };

  // transposed-read offsets (elements): lane 4q + p of a 16-lane group addresses row q,
  // columns 4p .. 4p + 3 of its 4 x 16 block and receives column fr of the four rows
  const int q = fr >> 2, p = fr & 3;
  const int rbase = 8 * (fg & 1) + 4 * (fg >> 1) + q;   // + 16 per read, + 32 per k-step
  int offD[TI], offX[NT][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int ch = wco * 2 * TI + 2 * i + (p >> 1);
    offD[i] = rbase * CO_T + ((ch ^ tr_key(rbase, CHD)) * 8) + 4 * (p & 1);
  }
#pragma unroll
  for (int dx = 0; dx < NT; ++dx)
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int ch = wci * 2 * TJ + 2 * j + (p >> 1);
      // the key reads bits 0..3 of the row: unchanged by the + 16 / + 32 of the reads
      offX[dx][j] = (rbase + dx) * CI_T + ((ch ^ tr_key(rbase + dx, CHX)) * 8) + 4 * (p & 1);
    }

  f32x4 acc[NT][TI][TJ];
#pragma unroll
  for (int dx = 0; dx < NT; ++dx)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j) acc[dx][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frag = [&](const bf16_t* base, int stride16) {
    const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)base);
    const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(base + stride16));
    bf16x8 f;
    f[0] = v0[0]; f[1] = v0[1]; f[2] = v0[2]; f[3] = v0[3];
    f[4] = v1[0]; f[5] = v1[1]; f[6] = v1[2]; f[7] = v1[3];
    return f;
  };
  auto compute = [&](int buf) {
    const bf16_t* tD = smem + buf * BUF_ELEMS;
    const bf16_t* tX = tD + D_ELEMS;
#pragma unroll
    for (int ks = 0; ks < WBK / 32; ++ks) {
      bf16x8 fd[TI];
#pragma unroll
      for (int i = 0; i < TI; ++i)
        fd[i] = frag(tD + offD[i] + ks * 32 * CO_T, 16 * CO_T);
#pragma unroll
      for (int dx = 0; dx < NT; ++dx)
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          const bf16x8 fx = frag(tX + offX[dx][j] + ks * 32 * CI_T, 16 * CI_T);
#pragma unroll
          for (int i = 0; i < TI; ++i)
            // acc[dx][i][j][reg] = dW[co 16 i + 4 fg + reg][tap dx][ci 16 j + fr]
            acc[dx][i][j] = mfma_16x16x32(fd[i], fx, acc[dx][i][j]);
        }
    }
  };

  if (s0 < s1) {   // workgroup-uniform; every lane stays active for the transposed reads
    dma(0, s0);
    __syncthreads();
    for (int st = s0; st < s1; ++st) {
      const int buf = (st - s0) & 1;
      if (st + 1 < s1) dma(buf ^ 1, st + 1);
      if (NZY == 0 && (st + 1) * WBK > M) {   // workgroup-uniform: the partial last slab
        zero_tail(buf, M - st * WBK);
        __syncthreads();
      }
      compute(buf);
      __syncthreads();   // next slab landed (vmcnt drained) and this one released
    }
  }

  // partial tile -> this split's slab [Cout][3 NZY][Cin], plain stores (64 B per 16 lanes)
  float* slab = ws + (int64_t)split * Cout * NSLAB * Cin;
#pragma unroll
  for (int dx = 0; dx < NT; ++dx)
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co_t * CO_T + wco * 16 * TI + 16 * i + 4 * fg + r;
          const int ci = ci_t * CI_T + wci * 16 * TJ + 16 * j + fr;
          slab[((int64_t)co * NSLAB + zy * NT + dx) * Cin + ci] = acc[dx][i][j][r];
        }
}

// dW = slab 0 + slab 1 + ... in index order
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float4* __restrict__ ws,
                                                      float4* __restrict__ dw, int64_t n4,
                                                      int split) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 s = ws[i];
  for (int k = 1; k < split; ++k) {
    const float4 v = ws[(int64_t)k * n4 + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  dw[i] = s;
}

// ------------------------------------------------------------------------- host half
struct WgradPlan { int wide, nco, nci, nsteps, split, sps; };

// M padded rows with `guard` guard rows on either side; NZY = 9 (3-D) or 3 (2-D)
// workgroups per (Cout, Cin) tile (NZY = 0, the linear layer: one, and no guard rows).
template <int NZY>
bool wgrad_plan(int64_t M, int64_t guard, int Cin, int Cout, WgradPlan* pl) {
  if (Cin % 64 != 0 || Cout % 64 != 0) return false;
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  // 32-bit byte offsets of the LDS DMA, as in conv3d.hip
  if ((M + 2 * guard) * cmax >= 0x3fffffffLL) return false;
  pl->wide = (Cin % 128 == 0 && Cout % 128 == 0) ? 1 : 0;
  const int tile = pl->wide ? 128 : 64;
  pl->nco = Cout / tile;
  pl->nci = Cin / tile;
  pl->nsteps = (int)((M + WBK - 1) / WBK);
  // Split over K: as many splits as keep NZY * tiles * split workgroups within ONE round
  // of the 256 CUs (one workgroup per CU: 48 accumulator tiles per wave), but at least 8
  // slabs of rows per split.  The Conv3d body (256 -> 256, M = 104 040): 36 tiles x 7 =
  // 252; the HSA ConvBlock (384 -> 384, M = 70 488): 27 tiles x 9 = 243.
  const int tiles = wgrad_groups(NZY) * pl->nco * pl->nci;
  int split = kNumCU / tiles;
  if (split > pl->nsteps / 8) split = pl->nsteps / 8;
  if (split < 1) split = 1;
  pl->sps = (pl->nsteps + split - 1) / split;
  pl->split = (pl->nsteps + pl->sps - 1) / pl->sps;   // no empty split
  return true;
}

// Bytes of the split-K slabs; -1: no plan for this shape.
template <int NZY>
int64_t wgrad_workspace_bytes(int64_t M, int64_t guard, int Cin, int Cout) {
  WgradPlan pl;
  if (!wgrad_plan<NZY>(M, guard, Cin, Cout, &pl)) return -1;
  return (int64_t)pl.split * Cout * (wgrad_taps(NZY) * wgrad_groups(NZY)) * Cin *
         (int64_t)sizeof(float);
}

template <int TI, int TJ, int NZY>
bool wgrad_launch(const WgradPlan& pl, const bf16_t* dy, const bf16_t* x, float* ws, int Yp,
                  int Xp, int Cin, int Cout, int M, hipStream_t s) {
  constexpr int lds = wgrad_lds_bytes(TI, TJ, wgrad_taps(NZY));
  static const hipError_t attr = hipFuncSetAttribute(   // once per instantiation
      reinterpret_cast<const void*>(&k_conv_k3_wgrad<TI, TJ, NZY>),
      hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) return false;
  const dim3 grid((unsigned)(wgrad_groups(NZY) * pl.nco * pl.nci), (unsigned)pl.split);
  hipLaunchKernelGGL((k_conv_k3_wgrad<TI, TJ, NZY>), grid, dim3(256), lds, s, dy, x, ws, Yp,
                     Xp, Cin, Cout, pl.nsteps, pl.sps, pl.nco, pl.nci, M);
  return true;
}

// dW [Cout][3 NZY][Cin] fp32 of padded rows dy, x (positive sizes, checked by the caller);
// NZY = 0: dW [Cout][Cin] of plain rows
template <int NZY>
int wgrad_run(const void* dy_padded, const void* x_padded, float* dw, void* workspace,
              int64_t workspace_bytes, int64_t M, int64_t guard, int Yp, int Xp, int Cin,
              int Cout, void* stream) {
  WgradPlan pl;
  if (!wgrad_plan<NZY>(M, guard, Cin, Cout, &pl)) return VEON_ERR_BAD_ARG;
  if (!dy_padded || !x_padded || !dw || !workspace || !al16(dy_padded) ||
      !al16(x_padded) || !al16(dw) || !al16(workspace))
    return VEON_ERR_BAD_ARG;
  const int64_t n = (int64_t)Cout * (wgrad_taps(NZY) * wgrad_groups(NZY)) * Cin;
  if (workspace_bytes < pl.split * n * (int64_t)sizeof(float)) return VEON_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bf16_t* D = static_cast<const bf16_t*>(dy_padded);
  const bf16_t* Xv = static_cast<const bf16_t*>(x_padded);
  float* ws = static_cast<float*>(workspace);
  if (!(pl.wide ? wgrad_launch<4, 4, NZY>(pl, D, Xv, ws, Yp, Xp, Cin, Cout, (int)M, s)
                : wgrad_launch<2, 2, NZY>(pl, D, Xv, ws, Yp, Xp, Cin, Cout, (int)M, s)))
    return VEON_ERR_LAUNCH;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0,
                     s, reinterpret_cast<const float4*>(ws), reinterpret_cast<float4*>(dw),
                     n / 4, pl.split);
  return launch_status();
}

}  // namespace
