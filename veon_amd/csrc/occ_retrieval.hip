// Open-vocabulary point retrieval on the occupancy path (the `retrieval=True` branch
// of VEONTemporal.simple_test, detectors/veon_temporal.py:232-241, 331-356, and
// SANInVeonTemporal, san_in_veon_temporal.py:195-200, 212, 268-273): the reference
// upsamples the head's C-channel feature volume to the evaluation grid in fp32
// (F.interpolate, trilinear, align_corners=False: 1.31 GB at C = 512), gathers it at
// the voxel of every LiDAR point (points_indices, datasets/pipelines/loading.py:
// 990-1012) and scores each point by F.cosine_similarity against a prompt embedding.
//
// Here the upsampled volume is never formed: every point blends the 8 low-resolution
// corner rows its output voxel interpolates from (the same ATen source-index rule as
// occ_tail.hip: src = scale*(dst+0.5)-0.5 clamped at 0, upper corner clamped at the
// edge), so only the rows the points touch are read, from the channels-last half
// rows of the sem head's PaddedVolume (interior only: never the halo or the guard
// rows) or from an fp32 volume of any strides.
//
// Structure: half a wave (32 lanes) owns one point, its lanes span the channels.
// Vector path (half rows, C % 8 == 0, 16-byte aligned rows): lane l holds channels
// 256k + 8l .. +8 for k < K, one 16-byte load per corner and chunk, all 8K loads of
// a lane in flight together.  Scalar path (fp32 any strides, or C % 8 != 0 /
// unaligned rows): lane l holds channels 32k + l.  The blend, |f|^2 and the Q dot
// products accumulate in fp32 per lane and are summed over the 32 lanes in registers
// (DPP row operations, then one v_permlane16_swap), in a fixed order: deterministic,
// no atomics.  The prompt norms are computed once per call by a small first kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_reduce.h"
#include "mfma_common.h"
#include "occ_interp.h"

namespace {

constexpr int kLanes = 32;   // lanes per point
constexpr int kPoints = 8;   // points per 256-thread workgroup
constexpr int kMaxC = 1024;  // channels a lane set holds in registers (32 floats per lane)

__device__ __forceinline__ float load_elem(const float* p) { return *p; }
__device__ __forceinline__ float load_elem(const bf16_t* p) { return bf2f(*p); }

// max(|e_q|, 1e-8) of every prompt row (one wave per prompt, fixed reduction order)
__global__ __launch_bounds__(64) void k_prompt_norms(const float* __restrict__ emb, int C,
                                                     float* __restrict__ norms) {
  const float* e = emb + (int64_t)blockIdx.x * C;
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 64) s += e[c] * e[c];
  // written out: through wave_sum (lane_reduce.h) the compiler schedules this kernel
  // differently, and the file is on the benchmark's path
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) norms[blockIdx.x] = fmaxf(sqrtf(s), 1e-8f);
}

// VEC: T = the build's half type, channel stride 1, 8 channels per lane and chunk;
// else lane l holds channels 32k + l.  K chunks (C <= K * 256 resp. K * 32).
template <typename T, bool VEC, int K>
__global__ __launch_bounds__(256) void k_occ_retrieve(
    const T* __restrict__ feat, Strides5 fs, int C, const float* __restrict__ bin,
    Strides5 bs, Grid g, const int* __restrict__ pts, int P,
    const float* __restrict__ emb, const float* __restrict__ enorm, int Q,
    float* __restrict__ score, float* __restrict__ bin_prob) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int p = blockIdx.x * kPoints + (threadIdx.x >> 5);
  if (p >= P) return;  // uniform over the half wave
  const int x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
  if (x < 0 || x >= g.Xo || y < 0 || y >= g.Yo || z < 0 || z >= g.Zo) {
    // outside the evaluation grid: NaN, nothing read
    if (lane == 0) {
      for (int q = 0; q < Q; ++q) score[(int64_t)q * P + p] = __builtin_nanf("");
      if (bin_prob) bin_prob[p] = __builtin_nanf("");
    }
    return;
  }
  const Axis az = source_clamped(z, g.scz, g.zi), ay = source_clamped(y, g.scy, g.yi),
             ax = source_clamped(x, g.scx, g.xi);
  int64_t off[8];
  corner_offsets(off, fs, az, ay, ax);

  constexpr int W = VEC ? 8 : 1;        // channels per lane and chunk
  constexpr int STEP = kLanes * W;      // channels per chunk
  float f[K][W];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = k * STEP + lane * W;
    if (ch < C) {
      if constexpr (VEC) {
        bf16x8 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          v[j] = *reinterpret_cast<const bf16x8*>(feat + off[j] + ch);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float c8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) c8[j] = bf2f((bf16_t)v[j][e]);
          f[k][e] = blend(c8, az, ay, ax);
        }
      } else {
        float c8[8];
        const T* fc = feat + (int64_t)ch * fs.c;
#pragma unroll
        for (int j = 0; j < 8; ++j) c8[j] = load_elem(fc + off[j]);
        f[k][0] = blend(c8, az, ay, ax);
      }
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) f[k][e] = 0.f;
    }
  }

  float sq = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < W; ++e) sq += f[k][e] * f[k][e];
  const float fnorm = fmaxf(sqrtf(half_wave_sum(sq)), 1e-8f);

  for (int q = 0; q < Q; ++q) {
    const float* eq = emb + (int64_t)q * C;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int ch = k * STEP + lane * W;
      if (ch < C) {
        if constexpr (VEC) {
          const float4 e0 = *reinterpret_cast<const float4*>(eq + ch);
          const float4 e1 = *reinterpret_cast<const float4*>(eq + ch + 4);
          d += f[k][0] * e0.x + f[k][1] * e0.y + f[k][2] * e0.z + f[k][3] * e0.w +
               f[k][4] * e1.x + f[k][5] * e1.y + f[k][6] * e1.z + f[k][7] * e1.w;
        } else {
          d += f[k][0] * eq[ch];
        }
      }
    }
    d = half_wave_sum(d);
    if (lane == 0) score[(int64_t)q * P + p] = d / (fnorm * enorm[q]);
  }

  if (bin_prob && lane == 0) {
    // softmax over (occupied, free) of the same interpolation of the two logits
    int64_t ob[8];
    corner_offsets(ob, bs, az, ay, ax);
    float c0[8], c1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c0[j] = bin[ob[j]];
      c1[j] = bin[ob[j] + bs.c];
    }
    const float o0 = blend(c0, az, ay, ax), o1 = blend(c1, az, ay, ax);
    const float om = o0 > o1 ? o0 : o1;
    const float e0 = expf(o0 - om), e1 = expf(o1 - om);
    bin_prob[p] = e0 / (e0 + e1);
  }
}

template <typename T, bool VEC, int K>
void launch(const T* feat, const Strides5& fs, int C, const float* bin, const Strides5& bs,
            const Grid& g, const int* pts, int P, const float* emb, const float* enorm,
            int Q, float* score, float* bin_prob, hipStream_t st) {
  const unsigned blocks = (unsigned)((P + kPoints - 1) / kPoints);
  hipLaunchKernelGGL((k_occ_retrieve<T, VEC, K>), dim3(blocks), dim3(256), 0, st, feat, fs,
                     C, bin, bs, g, pts, P, emb, enorm, Q, score, bin_prob);
}

template <typename T>
void launch_scalar(const T* feat, const Strides5& fs, int C, const float* bin,
                   const Strides5& bs, const Grid& g, const int* pts, int P,
                   const float* emb, const float* enorm, int Q, float* score,
                   float* bin_prob, hipStream_t st) {
  if (C <= kLanes)
    launch<T, false, 1>(feat, fs, C, bin, bs, g, pts, P, emb, enorm, Q, score, bin_prob, st);
  else if (C <= 4 * kLanes)
    launch<T, false, 4>(feat, fs, C, bin, bs, g, pts, P, emb, enorm, Q, score, bin_prob, st);
  else
    launch<T, false, kMaxC / kLanes>(feat, fs, C, bin, bs, g, pts, P, emb, enorm, Q, score,
                                     bin_prob, st);
}

}  // namespace

extern "C" int veon_occ_retrieve(const void* feat, int feat_is_half,
                                 const int64_t* feat_strides, int C, const float* bin,
                                 const int64_t* bin_strides, int B, int zi, int yi, int xi,
                                 int Zo, int Yo, int Xo, const int* points, int P, int batch,
                                 const float* emb, int Q, float* emb_norms, float* score,
                                 float* bin_prob, void* stream) {
  if (!feat || !feat_strides || !points || !emb || !emb_norms || !score ||
      (bin_prob && (!bin || !bin_strides)) || (feat_is_half != 0 && feat_is_half != 1) ||
      C <= 0 || C > kMaxC || Q < 1 || P < 0 || B <= 0 || batch < 0 || batch >= B ||
      zi <= 0 || yi <= 0 || xi <= 0 || Zo <= 0 || Yo <= 0 || Xo <= 0)
    return VEON_ERR_BAD_ARG;
  const unsigned esz = feat_is_half ? 2u : 4u;
  if (!aligned(feat, esz) || !aligned(points, 4) || !aligned(emb, 4) || !aligned(score, 4) ||
      (bin_prob && (!aligned(bin, 4) || !aligned(bin_prob, 4))) || !aligned(emb_norms, 4))
    return VEON_ERR_BAD_ARG;
  const int64_t* st = feat_strides;
  if (st[0] < 0 || st[1] <= 0 || st[2] < 0 || st[3] < 0 || st[4] < 0) return VEON_ERR_BAD_ARG;
  // channels-last rows: C may not run past the row into the next voxel
  if (st[1] == 1 && xi > 1 && C > st[4]) return VEON_ERR_BAD_ARG;
  if (bin_prob && (bin_strides[0] < 0 || bin_strides[1] < 0 || bin_strides[2] < 0 ||
                   bin_strides[3] < 0 || bin_strides[4] < 0))
    return VEON_ERR_BAD_ARG;
  if (P == 0) return VEON_OK;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_prompt_norms, dim3((unsigned)Q), dim3(64), 0, s, emb, C, emb_norms);
  const Strides5 fs = strides5(st);
  Strides5 bs{0, 0, 0, 0, 0};
  const float* bin_b = nullptr;
  if (bin_prob) {
    bs = strides5(bin_strides);
    bin_b = bin + batch * bs.b;
  }
  const Grid g{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
               (float)xi / (float)Xo};
  if (feat_is_half) {
    const bf16_t* fb = static_cast<const bf16_t*>(feat) + batch * fs.b;
    const bool vec = fs.c == 1 && C % 8 == 0 && aligned(fb, 16) && aligned(emb, 16) &&
                     fs.z % 8 == 0 && fs.y % 8 == 0 && fs.x % 8 == 0;
    if (vec) {
      const int K = (C + 255) / 256;
      if (K == 1)
        launch<bf16_t, true, 1>(fb, fs, C, bin_b, bs, g, points, P, emb, emb_norms, Q, score,
                                bin_prob, s);
      else if (K == 2)
        launch<bf16_t, true, 2>(fb, fs, C, bin_b, bs, g, points, P, emb, emb_norms, Q, score,
                                bin_prob, s);
      else if (K == 3)
        launch<bf16_t, true, 3>(fb, fs, C, bin_b, bs, g, points, P, emb, emb_norms, Q, score,
                                bin_prob, s);
      else
        launch<bf16_t, true, 4>(fb, fs, C, bin_b, bs, g, points, P, emb, emb_norms, Q, score,
                                bin_prob, s);
    } else {
      launch_scalar<bf16_t>(fb, fs, C, bin_b, bs, g, points, P, emb, emb_norms, Q, score,
                            bin_prob, s);
    }
  } else {
    launch_scalar<float>(static_cast<const float*>(feat) + batch * fs.b, fs, C, bin_b, bs, g,
                         points, P, emb, emb_norms, Q, score, bin_prob, s);
  }
  return launch_status();
}
