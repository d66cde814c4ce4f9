// The semantic tail of SAN's 2-D branch (SANInVeonTemporal.forward,
// san_in_veon_temporal.py:176-186, and semantic_inference_2d / _2d_w_embed, :240-255):
// class probabilities (softmax without the void column) and mask embeddings spread over
// the sigmoid of the Q mask proposals,
//
//   sem_seg_ds  [b,k,y,x] = sum_q cls[b,q,k]  * sigmoid(preds[b,q,y,x])          (h, w)
//   sem_embed_ds[b,c,y,x] = sum_q embs[b,q,c] * sigmoid(preds[b,q,y,x])          (h, w)
//   sem_seg     [b,k,Y,X] = sum_q cls[b,q,k]  * sigmoid(bilinear(preds[b,q])[Y,X])  (H, W)
//
// The reference forms bilinear(preds) and its sigmoid at (B,Q,H,W) first (two 1.7 GB
// tensors at six 512 x 1408 images and 100 proposals); here an upsampled proposal exists
// in one register, for as long as it takes to add it to the K class sums of its pixel.
//
//   k_sem2d_probs   cls = softmax(mask_logits)[..., :-1] -> the (B,Q,K) table, the only
//                   workspace; one wave per row
//   k_sem2d_ds      both low-resolution maps: one lane per pixel, one wave per 16 channels
//                   (the weights are wave-uniform: scalar loads)
//   k_sem2d_full    one lane per output pixel (PIX rows of it), K sums in registers; the
//                   class table and the few source pixels of the tile in LDS.  MAP stores
//                   the K sums; LABELS merges runs of rows by their maximum and stores the
//                   arg-max byte -- the same template, so the sums are the same bits
//
// Every sum over q runs q = 0, 1, ... with one fmaf per term; no atomics, no memset, every
// output element written.  Bilinear sampling is ATen's upsample_bilinear2d with
// align_corners=False (occ_interp.h `source`; its blend order w, then h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "class_runs.h"
#include "host_common.h"
#include "lane_reduce.h"
#include "occ_interp.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_Q = 256;
constexpr int TILE_W = 64;        // output columns of a tile: one per lane
constexpr int WAVES = THREADS / 64;
constexpr int TAB_FLOATS = 8192;  // LDS floats of the class table of one q chunk
constexpr int SRC_FLOATS = 4096;  // LDS floats of the source pixels of one q chunk
constexpr int DS_CH = 16;         // channels per wave of k_sem2d_ds

// 1 / (1 + 2^(-v * log2 e)) on the hardware's exp2 and reciprocal (1 ulp each; the product's
// rounding moves the result by less than |v| / 8 ulp): +-1e4 give exactly 1 and 0 (2^x
// overflows to inf and 1 / inf = 0; it underflows to 0 and 1 / 1 = 1), NaN stays NaN.
__device__ __forceinline__ float sigmoidf(float v) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.44269504088896341f));
}

// one wave per row of (B*Q, K+1) logits -> probs (B*Q, K)
__global__ __launch_bounds__(THREADS) void k_sem2d_probs(const float* __restrict__ logits,
                                                         int rows, int K,
                                                         float* __restrict__ probs) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* lp = logits + (int64_t)row * (K + 1);
  float v[MAX_ROWS / 64];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAX_ROWS / 64; ++i) {
    const int c = lane + 64 * i;
    v[i] = c <= K ? lp[c] : -INFINITY;
    m = fmaxf(m, v[i]);
  }
  m = wave_max(m);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAX_ROWS / 64; ++i) {
    v[i] = expf(v[i] - m);   // a column past K: expf(-inf) = 0
    s += v[i];
  }
  s = wave_sum(s);
  float* pp = probs + (int64_t)row * K;
#pragma unroll
  for (int i = 0; i < MAX_ROWS / 64; ++i) {
    const int c = lane + 64 * i;
    if (c < K) pp[c] = v[i] / s;
  }
}

// grid (ceil(P / 64), ceil(chunks / 4), B); wave -> one chunk of 16 channels of sem_seg_ds
// (weights: probs) or of sem_embed_ds (weights: embs), lane -> pixel
__global__ __launch_bounds__(THREADS) void k_sem2d_ds(
    const float* __restrict__ probs, const float* __restrict__ embs,
    const float* __restrict__ preds, int Q, int K, int C, int P, float* __restrict__ seg,
    float* __restrict__ emb) {
  const int lane = threadIdx.x & 63;
  const int chunk =
      __builtin_amdgcn_readfirstlane((int)(blockIdx.y * WAVES + (threadIdx.x >> 6)));
  const int nk = (K + DS_CH - 1) / DS_CH, nc = (C + DS_CH - 1) / DS_CH;
  if (chunk >= nk + nc) return;
  const int b = blockIdx.z;
  const bool is_seg = chunk < nk;
  const int n = is_seg ? K : C;
  int c0 = (is_seg ? chunk : chunk - nk) * DS_CH;
  // the last chunk of a row of 16 and more channels moves back to end with the row: its 16
  // weights are then one contiguous scalar load (channels it shares with the chunk before
  // are computed, and stored, twice with the same bits)
  if (n >= DS_CH && c0 > n - DS_CH) c0 = n - DS_CH;
  const float* wp = (is_seg ? probs : embs) + (int64_t)b * Q * n + c0;
  const int p = blockIdx.x * 64 + lane;
  const float* mp = preds + (int64_t)b * Q * P + (p < P ? p : P - 1);
  float acc[DS_CH];
#pragma unroll
  for (int e = 0; e < DS_CH; ++e) acc[e] = 0.f;
  if (n >= DS_CH) {
#pragma unroll 2   // (two proposals' loads in flight: the loop is latency-bound)
    for (int q = 0; q < Q; ++q) {
      const float s = sigmoidf(mp[(int64_t)q * P]);
      const float* wr = wp + (int64_t)q * n;
#pragma unroll
      for (int e = 0; e < DS_CH; ++e) acc[e] = fmaf(wr[e], s, acc[e]);
    }
  } else {   // a row shorter than a chunk: every accumulator's channel clamped into it
    for (int q = 0; q < Q; ++q) {
      const float s = sigmoidf(mp[(int64_t)q * P]);
      const float* wr = wp + (int64_t)q * n;
#pragma unroll
      for (int e = 0; e < DS_CH; ++e) acc[e] = fmaf(wr[e < n ? e : n - 1], s, acc[e]);
    }
  }
  if (p >= P) return;
  float* op = (is_seg ? seg : emb) + (int64_t)b * n * P + p;
#pragma unroll
  for (int e = 0; e < DS_CH; ++e)
    if (c0 + e < n) op[(int64_t)(c0 + e) * P] = acc[e];
}

struct FullArgs {
  const float* probs;   // (B,Q,K)
  const float* preds;   // (B,Q,h,w)
  int Q, K, h, w, H, W;
  float scy, scx;       // h / H, w / W in float, as ATen
  int QC;               // proposals per LDS chunk
  int RCAP;             // LDS floats per proposal for the tile's source pixels; 0: none
};

// One proposal onto the KACC sums of a lane's PIX pixels: sp is the proposal's source pixels
// (LDS or global memory), o00..o11 the offsets of each pixel's four taps in it, trow the
// proposal's KACC table values in LDS (zero past K; 16-byte aligned).  Straight-line: every
// table read is issued ahead of the multiply-adds.
template <int KACC, int PIX>
__device__ __forceinline__ void add_proposal(float (&acc)[PIX][KACC],
                                             const float* __restrict__ trow,
                                             const float* __restrict__ sp, const int* o00,
                                             const int* o01, const int* o10, const int* o11,
                                             const Axis& ax, const Axis* ay) {
  float s[PIX];
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    const float p00 = sp[o00[j]], p01 = sp[o01[j]], p10 = sp[o10[j]], p11 = sp[o11[j]];
    s[j] = sigmoidf(ay[j].l0 * (ax.l0 * p00 + ax.l1 * p01) +
                    ay[j].l1 * (ax.l0 * p10 + ax.l1 * p11));
  }
  const float4* t4 = reinterpret_cast<const float4*>(trow);
#pragma unroll
  for (int g = 0; g < KACC / 4; ++g) {
    const float4 t = t4[g];
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      acc[j][g * 4 + 0] = fmaf(t.x, s[j], acc[j][g * 4 + 0]);
      acc[j][g * 4 + 1] = fmaf(t.y, s[j], acc[j][g * 4 + 1]);
      acc[j][g * 4 + 2] = fmaf(t.z, s[j], acc[j][g * 4 + 2]);
      acc[j][g * 4 + 3] = fmaf(t.w, s[j], acc[j][g * 4 + 3]);
    }
  }
}

// grid (ceil(W / 64), ceil(H / (4 * PIX)), B).  Lane -> output column, wave -> PIX
// consecutive output rows.  KACC class sums per pixel live in registers; K > KACC takes
// ceil(K / KACC) passes over the proposals.  Per pass the proposals come in chunks of QC:
// their table rows [QC][KACC] and, with STAGED, the source pixels of the tile [QC][RCAP] are
// staged in LDS.  The host takes STAGED when RCAP floats hold the source pixels of any tile
// (`reach`); otherwise the taps are read from global memory, which changes no value.
// (the second launch bound, two waves per SIMD, keeps the scheduler from spending the
// whole register file on one wave)
template <int KACC, int PIX, bool LABELS, bool STAGED>
__global__ __launch_bounds__(THREADS, 2) void k_sem2d_full(
    FullArgs a, float* __restrict__ out, uint8_t* __restrict__ labels, GroupTable table,
    int grouped, int ignore_label) {
  extern __shared__ __align__(16) float smem[];
  __shared__ uint8_t gtab[MAX_ROWS];
  float* tab = smem;                       // [QC][KACC]
  float* srcl = smem + a.QC * KACC;        // [QC][RCAP]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (LABELS) gtab[threadIdx.x] = table.e[threadIdx.x];   // THREADS == MAX_ROWS
  static_assert(THREADS == MAX_ROWS, "one table byte per lane");
  const int b = blockIdx.z;
  const int ox0 = blockIdx.x * TILE_W, oy0 = blockIdx.y * (WAVES * PIX);
  const int ox1 = min(ox0 + TILE_W, a.W) - 1, oy1 = min(oy0 + WAVES * PIX, a.H) - 1;
  // the tile's source rectangle (`source` is monotone in dst)
  const int rx0 = source(ox0, a.scx, a.w).i0, ry0 = source(oy0, a.scy, a.h).i0;
  const int rw = source(ox1, a.scx, a.w).i1 - rx0 + 1;
  const int rh = source(oy1, a.scy, a.h).i1 - ry0 + 1;
  const int area = rw * rh;
  if (STAGED && area > a.RCAP) return;   // never: `reach` bounds rw and rh from above
  constexpr bool staged = STAGED;
  // this lane's pixels (clamped into the image: a lane outside computes and stores nothing)
  const int x = ox0 + lane;
  const Axis ax = source(min(x, a.W - 1), a.scx, a.w);
  Axis ay[PIX];
  int o00[PIX], o01[PIX], o10[PIX], o11[PIX];   // tap offsets within one proposal
#pragma unroll
  for (int j = 0; j < PIX; ++j) {
    ay[j] = source(min(oy0 + wave * PIX + j, a.H - 1), a.scy, a.h);
    const int sx0 = staged ? ax.i0 - rx0 : ax.i0, sx1 = staged ? ax.i1 - rx0 : ax.i1;
    const int sy0 = staged ? ay[j].i0 - ry0 : ay[j].i0, sy1 = staged ? ay[j].i1 - ry0 : ay[j].i1;
    const int pitch = staged ? rw : a.w;
    o00[j] = sy0 * pitch + sx0;
    o01[j] = sy0 * pitch + sx1;
    o10[j] = sy1 * pitch + sx0;
    o11[j] = sy1 * pitch + sx1;
  }
  const int hw = a.h * a.w;
  const float* pb = a.preds + (int64_t)b * a.Q * hw;
  const float* tb = a.probs + (int64_t)b * a.Q * a.K;
  RunArgMax best[PIX];   // (class_runs.h; MAX_ROWS there: the K + 1 logit columns)
  for (int k0 = 0; k0 < a.K; k0 += KACC) {
    const int kc = min(KACC, a.K - k0);
    float acc[PIX][KACC];
#pragma unroll
    for (int j = 0; j < PIX; ++j)
#pragma unroll
      for (int k = 0; k < KACC; ++k) acc[j][k] = 0.f;
    for (int q0 = 0; q0 < a.Q; q0 += a.QC) {
      const int qc = min(a.QC, a.Q - q0);
      __syncthreads();   // the previous chunk has been read
      for (int qi = wave; qi < qc; qi += WAVES) {
        const float* tr = tb + (int64_t)(q0 + qi) * a.K + k0;
        for (int k = lane; k < KACC; k += 64) tab[qi * KACC + k] = k < kc ? tr[k] : 0.f;
        if (staged) {
          const float* sp = pb + (int64_t)(q0 + qi) * hw + ry0 * a.w + rx0;
          for (int r = lane; r < area; r += 64) {
            const int yy = r / rw;
            srcl[qi * a.RCAP + r] = sp[yy * a.w + (r - yy * rw)];
          }
        }
      }
      __syncthreads();
#pragma unroll 1
      for (int qi = 0; qi < qc; ++qi)
        add_proposal<KACC, PIX>(acc, tab + qi * KACC,
                                staged ? srcl + qi * a.RCAP : pb + (int64_t)(q0 + qi) * hw, o00,
                                o01, o10, o11, ax, ay);
    }
    if (!LABELS) {
#pragma unroll
      for (int j = 0; j < PIX; ++j) {
        const int y = oy0 + wave * PIX + j;
        if (x < a.W && y < a.H) {
          float* op = out + (((int64_t)b * a.K + k0) * a.H + y) * a.W + x;
          const int64_t plane = (int64_t)a.H * a.W;
#pragma unroll
          for (int k = 0; k < KACC; ++k) {
            if (k < kc) *op = acc[j][k];
            op += plane;   // (one running address: k * plane would be KACC scalar pairs)
          }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < KACC; ++k) {
        if (k < kc) {
          const unsigned e = gtab[k0 + k];
          const int chan = grouped ? (int)(e & (RUN_ENDS - 1u)) : k0 + k;
          const bool ends = grouped ? (e & RUN_ENDS) != 0 : true;
#pragma unroll
          for (int j = 0; j < PIX; ++j) best[j].row(chan, ends, acc[j][k]);
        }
      }
    }
  }
  if (LABELS) {
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
      const int y = oy0 + wave * PIX + j;
      if (x < a.W && y < a.H)
        labels[((int64_t)b * a.H + y) * a.W + x] =
            (uint8_t)(best[j].bad || best[j].cls >= MAX_ROWS ? ignore_label : best[j].cls);
    }
  }
}

bool shape_ok(int B, int Q, int K, int h, int w) {
  return B > 0 && B <= 65535 && Q > 0 && Q <= MAX_Q && K > 0 && K + 1 <= MAX_ROWS && h > 0 &&
         w > 0 && (int64_t)h * w <= 0x7fffffffLL / MAX_Q;
}

void launch_probs(const float* logits, int B, int Q, int K, float* probs, hipStream_t st) {
  const int rows = B * Q;
  hipLaunchKernelGGL(k_sem2d_probs, dim3((unsigned)((rows + WAVES - 1) / WAVES)),
                     dim3(THREADS), 0, st, logits, rows, K, probs);
}

// Source pixels along one axis that `tile` consecutive output pixels can touch, from above:
// the first and the last pixel's fp32 source positions are (tile - 1) * in / out apart, up
// to 3 roundings of half an ulp of a position below 2^23 each (under 2 in all); the floor
// of the first, the upper tap of the last and the ceiling of the quotient add 3.
int reach(int tile, int in_size, int out_size) {
  const double need = (double)tile * in_size / out_size + 5.0;
  return need < in_size ? (int)need : in_size;
}

template <int KACC, int PIX, bool LABELS>
int launch_full(const float* probs, const float* preds, int B, int Q, int K, int h, int w,
                int H, int W, float* out, uint8_t* labels, const GroupTable& table,
                int grouped, int ignore_label, hipStream_t st) {
  const int tile_h = WAVES * PIX;
  const int64_t ty = ((int64_t)H + tile_h - 1) / tile_h;
  if (ty > 65535) return VEON_ERR_BAD_ARG;
  FullArgs a;
  a.probs = probs, a.preds = preds;
  a.Q = Q, a.K = K, a.h = h, a.w = w, a.H = H, a.W = W;
  // ATen: scale = in / out in float (area_pixel_compute_scale, no scale_factor given)
  a.scy = (float)h / (float)H, a.scx = (float)w / (float)W;
  a.QC = TAB_FLOATS / KACC < Q ? TAB_FLOATS / KACC : Q;
  const int64_t area = (int64_t)reach(tile_h, h, H) * reach(TILE_W, w, W);
  if (area <= SRC_FLOATS) {
    a.RCAP = (int)area;
    if (SRC_FLOATS / a.RCAP < a.QC) a.QC = SRC_FLOATS / a.RCAP;
  } else {
    a.RCAP = 0;
  }
  const size_t lds = (size_t)a.QC * (KACC + a.RCAP) * sizeof(float);
  const dim3 grid((unsigned)((W + TILE_W - 1) / TILE_W), (unsigned)ty, (unsigned)B);
  if (a.RCAP)
    hipLaunchKernelGGL((k_sem2d_full<KACC, PIX, LABELS, true>), grid, dim3(THREADS), lds, st,
                       a, out, labels, table, grouped, ignore_label);
  else
    hipLaunchKernelGGL((k_sem2d_full<KACC, PIX, LABELS, false>), grid, dim3(THREADS), lds, st,
                       a, out, labels, table, grouped, ignore_label);
  return launch_status();
}

// One instantiation per class of K: the more sums a pixel keeps, the fewer pixels a lane
// can hold, and every table value read from LDS (a broadcast: one float per clock and CU)
// should feed PIX * 64 multiply-adds.  20 x 4 covers the merged classes, 72 x 2 the
// detailed rows; 128 x 1 is the general case and is bound by the table reads.
template <bool LABELS>
int launch_full_for_k(const float* probs, const float* preds, int B, int Q, int K, int h,
                      int w, int H, int W, float* out, uint8_t* labels,
                      const GroupTable& table, int grouped, int ignore_label, hipStream_t st) {
  if (K <= 20)
    return launch_full<20, 4, LABELS>(probs, preds, B, Q, K, h, w, H, W, out, labels, table,
                                      grouped, ignore_label, st);
  if (K <= 72)
    return launch_full<72, 2, LABELS>(probs, preds, B, Q, K, h, w, H, W, out, labels, table,
                                      grouped, ignore_label, st);
  return launch_full<128, 1, LABELS>(probs, preds, B, Q, K, h, w, H, W, out, labels, table,
                                     grouped, ignore_label, st);
}

}  // namespace

extern "C" int veon_sem2d_ds(const float* mask_logits, const float* mask_embs,
                             const float* mask_preds, int B, int Q, int K, int C, int h, int w,
                             float* probs, float* sem_seg_ds, float* sem_embed_ds,
                             void* stream) {
  if (!mask_logits || !mask_preds || !probs || !sem_seg_ds || !shape_ok(B, Q, K, h, w) ||
      (mask_embs != nullptr) != (sem_embed_ds != nullptr) || (mask_embs && C <= 0))
    return VEON_ERR_BAD_ARG;
  if (!mask_embs) C = 0;
  const int P = h * w;
  const int64_t chunks = (K + DS_CH - 1) / DS_CH + ((int64_t)C + DS_CH - 1) / DS_CH;
  const int64_t gy = (chunks + WAVES - 1) / WAVES;
  if (gy > 65535) return VEON_ERR_BAD_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  launch_probs(mask_logits, B, Q, K, probs, st);
  hipLaunchKernelGGL(k_sem2d_ds, dim3((unsigned)((P + 63) / 64), (unsigned)gy, (unsigned)B),
                     dim3(THREADS), 0, st, probs, mask_embs, mask_preds, Q, K, C, P,
                     sem_seg_ds, sem_embed_ds);
  return launch_status();
}

extern "C" int veon_sem2d_full(const float* mask_logits, const float* mask_preds, int B, int Q,
                               int K, int h, int w, int H, int W, float* probs,
                               float* sem_seg, void* stream) {
  if (!mask_logits || !mask_preds || !probs || !sem_seg || !shape_ok(B, Q, K, h, w) ||
      H <= 0 || W <= 0)
    return VEON_ERR_BAD_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  launch_probs(mask_logits, B, Q, K, probs, st);
  const GroupTable none = {};
  return launch_full_for_k<false>(probs, mask_preds, B, Q, K, h, w, H, W, sem_seg, nullptr,
                                  none, 0, 0, st);
}

extern "C" int veon_sem2d_labels(const float* mask_logits, const float* mask_preds, int B,
                                 int Q, int K, int h, int w, int H, int W,
                                 const uint8_t* group, int n_merged, int ignore_label,
                                 float* probs, uint8_t* labels, void* stream) {
  if (!mask_logits || !mask_preds || !probs || !labels || !shape_ok(B, Q, K, h, w) ||
      H <= 0 || W <= 0 || ignore_label < 0 || ignore_label > 255)
    return VEON_ERR_BAD_ARG;
  GroupTable table = {};
  if (group && (n_merged <= 0 || n_merged > MAX_MERGED || !make_table(group, K, n_merged, &table)))
    return VEON_ERR_BAD_ARG;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  launch_probs(mask_logits, B, Q, K, probs, st);
  return launch_full_for_k<true>(probs, mask_preds, B, Q, K, h, w, H, W, nullptr, labels,
                                 table, group != nullptr, ignore_label, st);
}
