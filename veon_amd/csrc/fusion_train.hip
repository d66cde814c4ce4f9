// Training of the lift's 2-D fusion (CatFusionLift, semantic_net/layers.py:154-199) on
// token rows.  x1 (N, C1, H1, W1) and x2 (N, C2, H2, W2) are fp32 NCHW maps; M = N H W
// tokens of the lift's map, C = C1 + C2:
//     rc  = cat(resize(x1), resize(x2))   fp32 rows [M][C]         veon_fusion_resize_cat
//     xn1 = LN1(rc), xn2 = LN2(rc[:, C1:])  half rows               veon_fusion_dual_ln
//     y1  = relu(xn1 W1^T + b1), y2 = relu(xn2 W2^T + b2)  half     (veon_vit_gemm)
//     out = cat(y1, y2)                   fp32 rows [M][p1 + p2]    veon_fusion_join
// and backwards, given dout (fp32 rows):
//     dy1, dy2 = dout [y > 0]             half, padding columns 0   veon_fusion_relu_split
//     dW, db                              (veon_linear_wgrad_bf16, veon_rows_colsum_bf16)
//     dxn1 = dy1 W1, dxn2 = dy2 W2        half                      (veon_vit_gemm)
//     drc, dgamma / dbeta of both norms   fp32                      veon_fusion_dual_ln_bwd
//     dx1, dx2 = resize^T(drc)            fp32 NCHW                 veon_fusion_resize_adjoint
//
// The resize is torch's bilinear filter (align_corners = False, no antialias) from
// per-axis tables the host computes in fp32 once per shape pair, so that the forward, its
// adjoint and the tests' references index and weigh identically.  A table of an axis of
// `in` source and `out` destination positions is 3 out + 2 in 32-bit words:
//     i0[out] | i1[out] | l1[out] (float) | first[in] | last[in]
// destination d reads sources i0[d] and i1[d] with weights 1 - l1[d] and l1[d]; source s
// is read by the destinations first[s] <= d < last[s] and by no other (i0 is monotone, so
// they are one range).  Every index read from a table is clamped to its axis before it
// addresses anything.
//
// Both resize kernels transpose between NCHW (lanes along W) and rows (lanes along
// channels) through an LDS tile of 64 x 64 floats whose rows are padded to 65: a wave
// writes one row and reads one column, or the reverse, and both touch 64 different banks.
//
// No kernel here uses atomics or relies on a cleared output; every sum has a fixed order.
#include "mfma_common.h"
#include "ln_common.h"

namespace {

constexpr int kTile = 64;            // channels and positions of a transpose tile
constexpr int kTilePad = kTile + 1;  // floats per LDS row of it
constexpr int kDualBlocks = 512;     // partial sums of the dual LayerNorm backward (upper bound)
constexpr int kMaxC = 2048;          // widest concatenated row

struct AxisTable {
  const int* i0;
  const int* i1;
  const float* l1;
  const int* first;
  const int* last;
};

__host__ __device__ inline AxisTable axis_table(const void* t, int in, int out) {
  const int* p = static_cast<const int*>(t);
  AxisTable a;
  a.i0 = p;
  a.i1 = p + out;
  a.l1 = reinterpret_cast<const float*>(p + 2 * out);
  a.first = p + 3 * out;
  a.last = p + 3 * out + in;
  return a;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

// One input map of the forward: workgroup (bx, by, bz) blends the 64 channels bz of the
// destination positions x = 64 bx + 0..63 of row by = n H + y.  Phase one: wave w takes
// channels w, w + 4, ..., lane = x (NCHW reads along W).  Phase two: wave w takes
// positions w, w + 4, ..., lane = channel (256-byte row segments).
__global__ __launch_bounds__(256) void k_resize_rows(
    const float* __restrict__ x, float* __restrict__ rc, const void* __restrict__ taby,
    const void* __restrict__ tabx, int Cin, int Hin, int Win, int H, int W, int C, int coff,
    int identity) {
  __shared__ float tile[kTile][kTilePad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * kTile;
  const int n = blockIdx.y / H, y = blockIdx.y - n * H;
  const int c0 = blockIdx.z * kTile;
  const int dx = x0 + lane;
  if (dx < W) {
    int ya = y, yb = y, xa = dx, xb = dx;
    float ly = 0.f, lx = 0.f;
    if (!identity) {
      const AxisTable ty = axis_table(taby, Hin, H), tx = axis_table(tabx, Win, W);
      ya = clampi(ty.i0[y], 0, Hin - 1);
      yb = clampi(ty.i1[y], 0, Hin - 1);
      ly = ty.l1[y];
      xa = clampi(tx.i0[dx], 0, Win - 1);
      xb = clampi(tx.i1[dx], 0, Win - 1);
      lx = tx.l1[dx];
    }
    const float hy = 1.f - ly, hx = 1.f - lx;
    for (int c = wave; c < kTile; c += 4) {
      const float* p = x + ((int64_t)n * Cin + c0 + c) * Hin * Win;
      float v;
      if (identity) {
        v = p[(int64_t)y * Win + dx];
      } else {
        const float* pa = p + (int64_t)ya * Win;
        const float* pb = p + (int64_t)yb * Win;
        // torch's order: h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11)
        v = hy * (hx * pa[xa] + lx * pa[xb]) + ly * (hx * pb[xa] + lx * pb[xb]);
      }
      tile[c][lane] = v;
    }
  }
  __syncthreads();
  const int nx = W - x0 < kTile ? W - x0 : kTile;
  for (int j = wave; j < nx; j += 4)
    rc[((int64_t)blockIdx.y * W + x0 + j) * C + coff + c0 + lane] = tile[lane][j];
}

// One input map of the adjoint: workgroup (bx, by, bz) computes the 64 channels bz of the
// source positions sx = 64 bx + 0..63 of source row by = n Hin + sy.  Phase one: wave w
// takes positions w, w + 4, ..., lane = channel, and adds the destination tokens of the
// position's footprint, rows outside and columns inside, in index order.  Phase two:
// lane = sx, NCHW writes along W.  A position without a footprint is written as zero.
__global__ __launch_bounds__(256) void k_resize_adjoint(
    const float* __restrict__ drc, float* __restrict__ dx, const void* __restrict__ taby,
    const void* __restrict__ tabx, int Cin, int Hin, int Win, int H, int W, int C, int coff,
    int identity) {
  __shared__ float tile[kTile][kTilePad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s0 = blockIdx.x * kTile;
  const int n = blockIdx.y / Hin, sy = blockIdx.y - n * Hin;
  const int c0 = blockIdx.z * kTile;
  const int ns = Win - s0 < kTile ? Win - s0 : kTile;
  const float* src = drc + coff + c0 + lane;
  if (identity) {
    for (int j = wave; j < ns; j += 4)
      tile[lane][j] = src[(((int64_t)n * H + sy) * W + s0 + j) * C];
  } else {
    const AxisTable ty = axis_table(taby, Hin, H), tx = axis_table(tabx, Win, W);
    const int ya = clampi(ty.first[sy], 0, H), yb = clampi(ty.last[sy], 0, H);
    for (int j = wave; j < ns; j += 4) {
      const int sx = s0 + j;
      const int xa = clampi(tx.first[sx], 0, W), xb = clampi(tx.last[sx], 0, W);
      float acc = 0.f;
      for (int y = ya; y < yb; ++y) {
        const float ly = ty.l1[y];
        const float wy = (ty.i0[y] == sy ? 1.f - ly : 0.f) + (ty.i1[y] == sy ? ly : 0.f);
        const float* row = src + ((int64_t)n * H + y) * W * C;
        float racc = 0.f;
        for (int xx = xa; xx < xb; ++xx) {
          const float lx = tx.l1[xx];
          const float wx = (tx.i0[xx] == sx ? 1.f - lx : 0.f) + (tx.i1[xx] == sx ? lx : 0.f);
          racc = fmaf(wx, row[(int64_t)xx * C], racc);
        }
        acc = fmaf(wy, racc, acc);
      }
      tile[lane][j] = acc;
    }
  }
  __syncthreads();
  if (lane < ns)
    for (int c = wave; c < kTile; c += 4)
      dx[(((int64_t)n * Cin + c0 + c) * Hin + sy) * Win + s0 + lane] = tile[c][lane];
}

// A lane holds NCH float4 chunks of a row of C = 4 * nchunk floats: chunk lane + 64 h,
// h < NCH (NCH = ceil(C / 256), up to 8 for 2048 channels).  The chunks from q1 = C1 / 4 on
// are the row of the second LayerNorm.
template <int NCH>
__device__ __forceinline__ void load_chunks(const float* p, int lane, int nchunk, float4* v) {
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    v[h] = float4{0.f, 0.f, 0.f, 0.f};
    if (lane + 64 * h < nchunk) v[h] = reinterpret_cast<const float4*>(p)[lane + 64 * h];
  }
}

__device__ __forceinline__ float4 half4_to_float(const bf16_t* p) {
  const bf16x4 c = *reinterpret_cast<const bf16x4*>(p);
  return float4{bf2f((bf16_t)c[0]), bf2f((bf16_t)c[1]), bf2f((bf16_t)c[2]), bf2f((bf16_t)c[3])};
}

__device__ __forceinline__ void store_half4(bf16_t* p, float4 v) {
  bf16x4 o;
  o[0] = (short)f2bf(v.x); o[1] = (short)f2bf(v.y);
  o[2] = (short)f2bf(v.z); o[3] = (short)f2bf(v.w);
  *reinterpret_cast<bf16x4*>(p) = o;
}

// Two-pass statistics from registers (row_stats of ln_common.h on float4 chunks) of the
// chunks q0 <= chunk < nchunk: mean and rstd over the 4 (nchunk - q0) channels.
template <int NCH>
__device__ __forceinline__ void chunk_stats(const float4* v, int lane, int q0, int nchunk,
                                            float eps, float* mean, float* rstd) {
  const float cnt = 4.f * (nchunk - q0);
  float sum = 0.f;
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int q = lane + 64 * h;
    if (q >= q0 && q < nchunk) sum += (v[h].x + v[h].y) + (v[h].z + v[h].w);
  }
  *mean = wave_sum(sum) / cnt;
  float sq = 0.f;
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int q = lane + 64 * h;
    if (q >= q0 && q < nchunk) {
      const float a = v[h].x - *mean, b = v[h].y - *mean, c = v[h].z - *mean,
                  d = v[h].w - *mean;
      sq += (a * a + b * b) + (c * c + d * d);
    }
  }
  *rstd = rsqrtf(wave_sum(sq) / cnt + eps);
}

__device__ __forceinline__ float4 normed(float4 v, float mean, float rstd) {
  return float4{(v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd,
                (v.w - mean) * rstd};
}

__device__ __forceinline__ float4 affine(float4 xh, float4 g, float4 b) {
  return float4{fmaf(xh.x, g.x, b.x), fmaf(xh.y, g.y, b.y), fmaf(xh.z, g.z, b.z),
                fmaf(xh.w, g.w, b.w)};
}

// Forward: one wave per row, one read of the row, both normalisations from registers.
template <int NCH>
__global__ __launch_bounds__(256) void k_dual_ln(
    const float* __restrict__ rc, const float* __restrict__ g1, const float* __restrict__ b1,
    const float* __restrict__ g2, const float* __restrict__ b2, bf16_t* __restrict__ xn1,
    bf16_t* __restrict__ xn2, int M, int C1, int C2, float eps1, float eps2) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;   // wave-uniform
  const int C = C1 + C2, nchunk = C / 4, q1 = C1 / 4;
  float4 v[NCH];
  load_chunks<NCH>(rc + row * C, lane, nchunk, v);
  float m1, r1, m2, r2;
  chunk_stats<NCH>(v, lane, 0, nchunk, eps1, &m1, &r1);
  chunk_stats<NCH>(v, lane, q1, nchunk, eps2, &m2, &r2);
#pragma unroll
  for (int h = 0; h < NCH; ++h) {
    const int q = lane + 64 * h;
    if (q >= nchunk) continue;
    const float4 o1 = affine(normed(v[h], m1, r1), reinterpret_cast<const float4*>(g1)[q],
                             reinterpret_cast<const float4*>(b1)[q]);
    store_half4(xn1 + row * C + 4 * q, o1);
    if (q >= q1) {
      const float4 o2 = affine(normed(v[h], m2, r2),
                               reinterpret_cast<const float4*>(g2)[q - q1],
                               reinterpret_cast<const float4*>(b2)[q - q1]);
      store_half4(xn2 + row * C2 + 4 * (q - q1), o2);
    }
  }
}

__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}

__device__ __forceinline__ float sum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }

__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
  return float4{a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w};
}

__device__ __forceinline__ void add4(float4* a, float4 b) {
  a->x += b.x; a->y += b.y; a->z += b.z; a->w += b.w;
}

// dx = rstd (a - mean(a) - xhat mean(a xhat)), a = dout gamma
__device__ __forceinline__ float4 ln_dx(float4 a, float4 xh, float s1, float s2, float rstd) {
  return float4{rstd * (a.x - s1 - xh.x * s2), rstd * (a.y - s1 - xh.y * s2),
                rstd * (a.z - s1 - xh.z * s2), rstd * (a.w - s1 - xh.w * s2)};
}

// Backward, stage one of the parameter sums.  Workgroup b walks rows [b rows_per_block,
// (b + 1) rows_per_block), wave w of it rows w, w + 4, ...; the statistics of both norms
// are recomputed from the row, drc is written once (its x2 columns as the sum of both
// branches), and every lane keeps four running sums per chunk: dgamma1, dbeta1, dgamma2,
// dbeta2.  At the end the waves are added in wave order, one kind of sum at a time
// through the same LDS buffer, and part[b] = [dgamma1 C | dbeta1 C | dgamma2 C2 | dbeta2
// C2] is written.
template <int NCH>
__global__ __launch_bounds__(256) void k_dual_ln_bwd(
    const bf16_t* __restrict__ dxn1, const bf16_t* __restrict__ dxn2,
    const float* __restrict__ rc, const float* __restrict__ g1, const float* __restrict__ g2,
    float* __restrict__ drc, float* __restrict__ part, int M, int C1, int C2, float eps1,
    float eps2, int rows_per_block) {
  __shared__ float4 red[3][NCH * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = C1 + C2, nchunk = C / 4, q1 = C1 / 4;
  float4 acc[4][NCH];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int h = 0; h < NCH; ++h) acc[s][h] = float4{0.f, 0.f, 0.f, 0.f};
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  for (int64_t m = r0 + wave; m < r1; m += 4) {
    float4 v[NCH], d1[NCH], d2[NCH];
    load_chunks<NCH>(rc + m * C, lane, nchunk, v);
    float mean1, rstd1, mean2, rstd2;
    chunk_stats<NCH>(v, lane, 0, nchunk, eps1, &mean1, &rstd1);
    chunk_stats<NCH>(v, lane, q1, nchunk, eps2, &mean2, &rstd2);
    float s11 = 0.f, s12 = 0.f, s21 = 0.f, s22 = 0.f;
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int q = lane + 64 * h;
      d1[h] = d2[h] = float4{0.f, 0.f, 0.f, 0.f};
      if (q >= nchunk) continue;
      d1[h] = half4_to_float(dxn1 + m * C + 4 * q);
      const float4 xh = normed(v[h], mean1, rstd1);
      const float4 a = mul4(d1[h], reinterpret_cast<const float4*>(g1)[q]);
      s11 += sum4(a);
      s12 += dot4(a, xh);
      add4(&acc[0][h], mul4(d1[h], xh));
      add4(&acc[1][h], d1[h]);
      if (q >= q1) {
        d2[h] = half4_to_float(dxn2 + m * C2 + 4 * (q - q1));
        const float4 xh2 = normed(v[h], mean2, rstd2);
        const float4 a2 = mul4(d2[h], reinterpret_cast<const float4*>(g2)[q - q1]);
        s21 += sum4(a2);
        s22 += dot4(a2, xh2);
        add4(&acc[2][h], mul4(d2[h], xh2));
        add4(&acc[3][h], d2[h]);
      }
    }
    s11 = wave_sum(s11) / C;
    s12 = wave_sum(s12) / C;
    s21 = wave_sum(s21) / C2;
    s22 = wave_sum(s22) / C2;
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
      const int q = lane + 64 * h;
      if (q >= nchunk) continue;
      float4 o = ln_dx(mul4(d1[h], reinterpret_cast<const float4*>(g1)[q]),
                       normed(v[h], mean1, rstd1), s11, s12, rstd1);
      if (q >= q1)
        add4(&o, ln_dx(mul4(d2[h], reinterpret_cast<const float4*>(g2)[q - q1]),
                       normed(v[h], mean2, rstd2), s21, s22, rstd2));
      reinterpret_cast<float4*>(drc + m * C)[q] = o;
    }
  }
  float* out = part + (int64_t)blockIdx.x * (2 * C + 2 * C2);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    park_waves<NCH>(acc[s], red, lane, wave);
    if (wave == 0) {
      // sums 0, 1 span the whole row, sums 2, 3 the chunks from q1 on
      float* o = out + (s < 2 ? s * C : 2 * C + (s - 2) * C2);
#pragma unroll
      for (int h = 0; h < NCH; ++h) {
        const int q = lane + 64 * h;
        if (q >= nchunk || (s >= 2 && q < q1)) continue;
        reinterpret_cast<float4*>(o)[s < 2 ? q : q - q1] =
            add_waves_in_order(acc[s][h], red, h * 64 + lane);
      }
    }
    __syncthreads();
  }
}

// out fp32 [M][p1 + p2] = cat(y1[:, :p1], y2[:, :p2]) of half rows of ld1 / ld2 columns:
// four columns per thread.
__global__ __launch_bounds__(256) void k_join(const bf16_t* __restrict__ y1,
                                              const bf16_t* __restrict__ y2,
                                              float* __restrict__ out, int64_t n4, int p1,
                                              int p2, int ld1, int ld2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int q = (p1 + p2) / 4;
  const int64_t m = i / q;
  const int c = (int)(i - m * q) * 4;
  const bf16_t* p = c < p1 ? y1 + m * ld1 + c : y2 + m * ld2 + (c - p1);
  reinterpret_cast<float4*>(out)[i] = half4_to_float(p);
}

// dy1 half [M][ld1], dy2 half [M][ld2] = dout where the stored ReLU output is positive,
// zero elsewhere and in the padding columns: four columns of [dy1 | dy2] per thread.
__global__ __launch_bounds__(256) void k_relu_split(
    const float* __restrict__ dout, const bf16_t* __restrict__ y1,
    const bf16_t* __restrict__ y2, bf16_t* __restrict__ dy1, bf16_t* __restrict__ dy2,
    int64_t n4, int p1, int p2, int ld1, int ld2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int q = (ld1 + ld2) / 4;
  const int64_t m = i / q;
  int c = (int)(i - m * q) * 4;
  const bool second = c >= ld1;
  if (second) c -= ld1;
  const int p = second ? p2 : p1, ld = second ? ld2 : ld1;
  float4 g = {0.f, 0.f, 0.f, 0.f};
  if (c < p) {
    const float4 y = half4_to_float((second ? y2 : y1) + m * ld + c);
    const float4 d =
        *reinterpret_cast<const float4*>(dout + m * (p1 + p2) + (second ? p1 : 0) + c);
    g = float4{y.x > 0.f ? d.x : 0.f, y.y > 0.f ? d.y : 0.f, y.z > 0.f ? d.z : 0.f,
               y.w > 0.f ? d.w : 0.f};
  }
  store_half4((second ? dy2 : dy1) + m * ld + c, g);
}

bool dual_widths_ok(int C1, int C2) {
  return C1 > 0 && C2 > 0 && C1 % 64 == 0 && C2 % 64 == 0 && C1 + C2 <= kMaxC;
}

bool fits31(int64_t a, int64_t b, int64_t c, int64_t d) {
  return a * b <= 0x7fffffffLL / (c * d);
}

// grid and range checks shared by the two resize entry points
bool resize_args_ok(const void* x, const void* rows, const void* taby, const void* tabx,
                    int N, int Cin, int Hin, int Win, int H, int W, int C, int coff) {
  if (!x || !rows || N <= 0 || Cin <= 0 || Cin % kTile != 0 || Hin <= 0 || Win <= 0 ||
      H <= 0 || W <= 0 || C <= 0 || C % 4 != 0 || coff < 0 || coff % 4 != 0 ||
      coff + Cin > C || !al16(x) || !al16(rows))
    return false;
  const bool identity = Hin == H && Win == W;
  if (!identity && (!taby || !tabx || !al16(taby) || !al16(tabx))) return false;
  // element counts within 31 bits, grid dimensions y and z within 65535
  if (!fits31(N, Cin, Hin, Win) || !fits31(N, H, W, C)) return false;
  if ((int64_t)N * H > 65535 || (int64_t)N * Hin > 65535 || Cin / kTile > 65535) return false;
  return true;
}

}  // namespace

extern "C" {

int veon_fusion_resize_cat(const float* x, float* rc, const void* taby, const void* tabx,
                           int N, int Cin, int Hin, int Win, int H, int W, int C, int coff,
                           void* stream) {
  if (!resize_args_ok(x, rc, taby, tabx, N, Cin, Hin, Win, H, W, C, coff))
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_resize_rows,
                     dim3((unsigned)((W + kTile - 1) / kTile), (unsigned)(N * H),
                          (unsigned)(Cin / kTile)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), x, rc, taby, tabx, Cin,
                     Hin, Win, H, W, C, coff, (Hin == H && Win == W) ? 1 : 0);
  return launch_status();
}

int veon_fusion_resize_adjoint(const float* drc, float* dx, const void* taby,
                               const void* tabx, int N, int Cin, int Hin, int Win, int H,
                               int W, int C, int coff, void* stream) {
  if (!resize_args_ok(dx, drc, taby, tabx, N, Cin, Hin, Win, H, W, C, coff) || drc == dx)
    return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_resize_adjoint,
                     dim3((unsigned)((Win + kTile - 1) / kTile), (unsigned)(N * Hin),
                          (unsigned)(Cin / kTile)),
                     dim3(256), 0, static_cast<hipStream_t>(stream), drc, dx, taby, tabx, Cin,
                     Hin, Win, H, W, C, coff, (Hin == H && Win == W) ? 1 : 0);
  return launch_status();
}

#define VEON_DUAL_SWITCH(C, LAUNCH)            \
  switch (((C) + 255) / 256) {                 \
    case 1: LAUNCH(1); break;                  \
    case 2: LAUNCH(2); break;                  \
    case 3: LAUNCH(3); break;                  \
    case 4: LAUNCH(4); break;                  \
    case 5: LAUNCH(5); break;                  \
    case 6: LAUNCH(6); break;                  \
    case 7: LAUNCH(7); break;                  \
    default: LAUNCH(8); break;                 \
  }

int veon_fusion_dual_ln(const float* rc, const float* gamma1, const float* beta1,
                        const float* gamma2, const float* beta2, void* xn1, void* xn2, int M,
                        int C1, int C2, float eps1, float eps2, void* stream) {
  if (M <= 0 || !dual_widths_ok(C1, C2) || !rc || !gamma1 || !beta1 || !gamma2 || !beta2 ||
      !xn1 || !xn2 || !al16(rc) || !al16(gamma1) || !al16(beta1) || !al16(gamma2) ||
      !al16(beta2) || !al16(xn1) || !al16(xn2) ||
      (int64_t)M * (C1 + C2) > 0x7fffffffLL)
    return VEON_ERR_BAD_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
#define VEON_DUAL_FWD(K)                                                                    \
  hipLaunchKernelGGL((k_dual_ln<K>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, rc,    \
                     gamma1, beta1, gamma2, beta2, static_cast<bf16_t*>(xn1),               \
                     static_cast<bf16_t*>(xn2), M, C1, C2, eps1, eps2)
  VEON_DUAL_SWITCH(C1 + C2, VEON_DUAL_FWD)
#undef VEON_DUAL_FWD
  return launch_status();
}

int64_t veon_fusion_dual_ln_bwd_workspace_bytes(int C1, int C2) {
  if (!dual_widths_ok(C1, C2)) return -1;
  return (int64_t)kDualBlocks * (2 * (C1 + C2) + 2 * C2) * (int64_t)sizeof(float);
}

int veon_fusion_dual_ln_bwd(const void* dxn1, const void* dxn2, const float* rc,
                            const float* gamma1, const float* gamma2, float* drc,
                            float* sums, void* workspace, int64_t workspace_bytes, int M,
                            int C1, int C2, float eps1, float eps2, void* stream) {
  if (M <= 0 || !dual_widths_ok(C1, C2) || !dxn1 || !dxn2 || !rc || !gamma1 || !gamma2 ||
      !drc || !sums || !workspace || drc == rc || !al16(dxn1) || !al16(dxn2) || !al16(rc) ||
      !al16(gamma1) || !al16(gamma2) || !al16(drc) || !al16(sums) || !al16(workspace) ||
      (int64_t)M * (C1 + C2) > 0x7fffffffLL)
    return VEON_ERR_BAD_ARG;
  if (workspace_bytes < veon_fusion_dual_ln_bwd_workspace_bytes(C1, C2))
    return VEON_ERR_WORKSPACE;
  // at least two rounds of rows per workgroup, at most kDualBlocks workgroups
  int rows = (M + kDualBlocks - 1) / kDualBlocks;
  if (rows < 8) rows = 8;
  const int nblocks = (M + rows - 1) / rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
#define VEON_DUAL_BWD(K)                                                                    \
  hipLaunchKernelGGL((k_dual_ln_bwd<K>), dim3(nblocks), dim3(256), 0, s,                    \
                     static_cast<const bf16_t*>(dxn1), static_cast<const bf16_t*>(dxn2), rc, \
                     gamma1, gamma2, drc, part, M, C1, C2, eps1, eps2, rows)
  VEON_DUAL_SWITCH(C1 + C2, VEON_DUAL_BWD)
#undef VEON_DUAL_BWD
  const int n4 = (2 * (C1 + C2) + 2 * C2) / 4;
  hipLaunchKernelGGL(k_ln_sums_final, dim3((n4 + 3) / 4), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(part), reinterpret_cast<float4*>(sums),
                     n4, nblocks);
  return launch_status();
}

#undef VEON_DUAL_SWITCH

static bool join_args_ok(int M, int p1, int p2, int ld1, int ld2) {
  return M > 0 && p1 > 0 && p2 > 0 && p1 % 4 == 0 && p2 % 4 == 0 && ld1 >= p1 && ld2 >= p2 &&
         ld1 % 8 == 0 && ld2 % 8 == 0 && (int64_t)M * (ld1 + ld2) <= 0x7fffffffLL;
}

int veon_fusion_join(const void* y1, const void* y2, float* out, int M, int p1, int p2,
                     int ld1, int ld2, void* stream) {
  if (!join_args_ok(M, p1, p2, ld1, ld2) || !y1 || !y2 || !out || !al16(y1) || !al16(y2) ||
      !al16(out))
    return VEON_ERR_BAD_ARG;
  const int64_t n4 = (int64_t)M * ((p1 + p2) / 4);
  hipLaunchKernelGGL(k_join, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(y1),
                     static_cast<const bf16_t*>(y2), out, n4, p1, p2, ld1, ld2);
  return launch_status();
}

int veon_fusion_relu_split(const float* dout, const void* y1, const void* y2, void* dy1,
                           void* dy2, int M, int p1, int p2, int ld1, int ld2,
                           void* stream) {
  if (!join_args_ok(M, p1, p2, ld1, ld2) || !dout || !y1 || !y2 || !dy1 || !dy2 ||
      !al16(dout) || !al16(y1) || !al16(y2) || !al16(dy1) || !al16(dy2))
    return VEON_ERR_BAD_ARG;
  const int64_t n4 = (int64_t)M * ((ld1 + ld2) / 4);
  hipLaunchKernelGGL(k_relu_split, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), dout,
                     static_cast<const bf16_t*>(y1), static_cast<const bf16_t*>(y2),
                     static_cast<bf16_t*>(dy1), static_cast<bf16_t*>(dy2), n4, p1, p2, ld1,
                     ld2);
  return launch_status();
}

}  // extern "C"
