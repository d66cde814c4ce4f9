// The differentiable primitive of VEON's 2D->3D feature-alignment loss
// (Proj2Dto3DLoss, models/semantic_net/loss/occ_loss_utils/occ3d_nuscenes.py:454-461,
// 497-504): for every entry i = (voxel_i, label_i), the cosine between the trilinearly
// upsampled feature at the voxel and row label_i of the class-embedding table.  The
// reference upsamples feat_occ to (B, C, 16, 200, 200) fp32 (1.31 GB at C = 512,
// san_in_veon_temporal.py:196-200), permutes and reshapes it (a second copy) and
// autograd keeps a gradient of that size for each.  Here the upsampled volume is formed
// in neither direction.
//
// Forward (k_align_fwd): as k_occ_retrieve's fp32 path, half a wave per entry, lanes
// across channels, the 8 corner rows blended in registers, fixed-order DPP reductions;
// one table row per entry.  It also stores <f, t>/max(|t|, eps) and |f| per entry.
//
// Backward of sum_i g_i cos_i: store-and-sum over a FIXED inverted index, no atomics.
// For the 2x upsampling VEON uses, low-resolution voxel j receives only from output
// voxels 2j-1 .. 2j+2 per axis (64 candidates).
//   pass A (k_align_rows): half a wave per DISTINCT output voxel re-blends f, sums its
//     entries' g_i * d cos_i / d f in entry order and stores one fp32 gradient row;
//   pass B (k_align_gather): half a wave per low-resolution voxel walks its 64
//     candidates in a fixed order, looks each up in a dense occ -> row table and adds
//     w * row for those present; one plain store per element, zeros where the
//     neighbourhood is empty, so the result needs no memset and is bit-reproducible.
// No half operands: the file is identical in both library flavours.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_reduce.h"
#include "mfma_common.h"
#include "occ_interp.h"

namespace {

constexpr int kLanes = 32;    // lanes per entry / voxel
constexpr int kPerWG = 8;     // entries / voxels per 256-thread workgroup
constexpr int kMaxC = 1024;   // channels a lane set holds in registers (32 floats per lane)

// W consecutive channels of one row (W = 4: one 16-byte access)
template <int W>
__device__ __forceinline__ void load_w(const float* p, float* v) {
  if constexpr (W == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void store_w(float* p, const float* v) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// max(|t_k|, eps) of every table row (one wave per row, fixed reduction order)
__global__ __launch_bounds__(64) void k_table_norms(const float* __restrict__ table, int C,
                                                    float eps, float* __restrict__ norms) {
  const float* e = table + (int64_t)blockIdx.x * C;
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 64) s += e[c] * e[c];
  s = wave_sum(s);
  if (threadIdx.x == 0) norms[blockIdx.x] = fmaxf(sqrtf(s), eps);
}

// f[k][e] = the trilinear blend at one output voxel of channels (k * 32 + lane) * W + e.
// W = 4: channel stride 1, 16-byte aligned rows; W = 1: any strides.
template <int W, int K>
__device__ __forceinline__ void blend_rows(const float* __restrict__ feat, const Strides5& fs,
                                           int C, int lane, const Axis& az, const Axis& ay,
                                           const Axis& ax, float (&f)[K][W]) {
  int64_t off[8];
  corner_offsets(off, fs, az, ay, ax);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = (k * kLanes + lane) * W;
    if (ch < C) {
      float v[8][W];
      const float* fc = feat + (W == 4 ? (int64_t)ch : (int64_t)ch * fs.c);
#pragma unroll
      for (int j = 0; j < 8; ++j) load_w<W>(fc + off[j], v[j]);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        float c8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) c8[j] = v[j][e];
        f[k][e] = blend(c8, az, ay, ax);
      }
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) f[k][e] = 0.f;
    }
  }
}

template <int W, int K>
__global__ __launch_bounds__(256) void k_align_fwd(
    const float* __restrict__ feat, Strides5 fs, int C, Grid g, const int* __restrict__ vox,
    const int* __restrict__ labels, int N, const float* __restrict__ table,
    const float* __restrict__ tnorm, int nrows, float eps, float* __restrict__ cos_out,
    float* __restrict__ stats) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int i = blockIdx.x * kPerWG + (threadIdx.x >> 5);
  if (i >= N) return;  // uniform over the half wave
  const int x = vox[3 * i], y = vox[3 * i + 1], z = vox[3 * i + 2];
  const int lab = labels[i];
  if (x < 0 || x >= g.Xo || y < 0 || y >= g.Yo || z < 0 || z >= g.Zo || lab < 0 ||
      lab >= nrows) {
    // the host refuses such entries before the launch; nothing is read for them here
    if (lane == 0) {
      cos_out[i] = 0.f;
      stats[2 * i] = 0.f;
      stats[2 * i + 1] = 0.f;
    }
    return;
  }
  const Axis az = source_clamped(z, g.scz, g.zi), ay = source_clamped(y, g.scy, g.yi),
             ax = source_clamped(x, g.scx, g.xi);
  float f[K][W];
  blend_rows<W, K>(feat, fs, C, lane, az, ay, ax, f);

  const float* t = table + (int64_t)lab * C;
  float sq = 0.f, d = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = (k * kLanes + lane) * W;
    if (ch < C) {
      float tv[W];
      load_w<W>(t + ch, tv);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        sq += f[k][e] * f[k][e];
        d += f[k][e] * tv[e];
      }
    }
  }
  const float fn = sqrtf(half_wave_sum(sq));
  d = half_wave_sum(d);
  if (lane == 0) {
    const float du = d / tnorm[lab];
    cos_out[i] = du / fmaxf(fn, eps);
    stats[2 * i] = du;
    stats[2 * i + 1] = fn;
  }
}

// Pass A.  Row m = sum over the entries e of distinct voxel m, in the order given, of
//   g_e * (u_e / n - (<f, u_e> / n^2) * f / |f|),  n = max(|f|, eps), u_e = t_e / max(|t_e|, eps)
// (the last factor 0 at f = 0): what autograd returns for ATen's cosine_similarity,
// whose clamp is applied under a no-grad guard.
template <int W, int K>
__global__ __launch_bounds__(256) void k_align_rows(
    const float* __restrict__ feat, Strides5 fs, int C, Grid g, const int* __restrict__ vox,
    const int* __restrict__ labels, int N, const float* __restrict__ table,
    const float* __restrict__ tnorm, int nrows, float eps, const float* __restrict__ stats,
    const float* __restrict__ gout, const int* __restrict__ order,
    const int* __restrict__ seg, int M, float* __restrict__ rows) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int m = blockIdx.x * kPerWG + (threadIdx.x >> 5);
  if (m >= M) return;
  int e0 = seg[m], e1 = seg[m + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > N ? N : e1;
  float acc[K][W];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < W; ++e) acc[k][e] = 0.f;

  int first = e0 < e1 ? order[e0] : -1;
  bool ok = first >= 0 && first < N;
  int x = 0, y = 0, z = 0;
  if (ok) {
    x = vox[3 * first]; y = vox[3 * first + 1]; z = vox[3 * first + 2];
    ok = x >= 0 && x < g.Xo && y >= 0 && y < g.Yo && z >= 0 && z < g.Zo;
  }
  if (ok) {
    const Axis az = source_clamped(z, g.scz, g.zi), ay = source_clamped(y, g.scy, g.yi),
               ax = source_clamped(x, g.scx, g.xi);
    float f[K][W];
    blend_rows<W, K>(feat, fs, C, lane, az, ay, ax, f);
    for (int e = e0; e < e1; ++e) {
      const int i = order[e];
      if (i < 0 || i >= N) continue;
      const int lab = labels[i];
      if (lab < 0 || lab >= nrows) continue;
      const float gi = gout[i], du = stats[2 * i], fn = stats[2 * i + 1];
      const float n = fmaxf(fn, eps);
      const float a = gi / (n * tnorm[lab]);
      const float b = fn > 0.f ? gi * du / (n * n * fn) : 0.f;
      const float* t = table + (int64_t)lab * C;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int ch = (k * kLanes + lane) * W;
        if (ch < C) {
          float tv[W];
          load_w<W>(t + ch, tv);
#pragma unroll
          for (int w = 0; w < W; ++w) acc[k][w] += a * tv[w] - b * f[k][w];
        }
      }
    }
  }
  float* r = rows + (int64_t)m * C;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = (k * kLanes + lane) * W;
    if (ch < C) store_w<W>(r + ch, acc[k]);
  }
}

// Pass B (2x per axis).  grad: (zi, yi, xi, C) contiguous, every element stored once.
template <int W, int K>
__global__ __launch_bounds__(256) void k_align_gather(
    const float* __restrict__ rows, int M, const int* __restrict__ occ_rows, int C, Grid g,
    float* __restrict__ grad) {
  const int lane = threadIdx.x & (kLanes - 1);
  const int64_t j = (int64_t)blockIdx.x * kPerWG + (threadIdx.x >> 5);
  const int64_t nlow = (int64_t)g.zi * g.yi * g.xi;
  if (j >= nlow) return;
  const int jx = (int)(j % g.xi), jy = (int)((j / g.xi) % g.yi), jz = (int)(j / ((int64_t)g.xi * g.yi));
  // lane l looks candidates l and l + 32 up; candidate c = (tz, ty, tx) = (c/16, c/4%4, c%4)
  int mrow[2];
  float wgt[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 32 * h;
    const int oz = 2 * jz - 1 + (c >> 4), oy = 2 * jy - 1 + ((c >> 2) & 3),
              ox = 2 * jx - 1 + (c & 3);
    const float w = axis_weight(oz, g.Zo, jz, g.scz, g.zi) *
                    axis_weight(oy, g.Yo, jy, g.scy, g.yi) *
                    axis_weight(ox, g.Xo, jx, g.scx, g.xi);
    int m = -1;
    if (w != 0.f) {   // zero weight: outside the grid or a corner that does not reach j
      m = occ_rows[((int64_t)oz * g.Yo + oy) * g.Xo + ox];
      if (m >= M) m = -1;
    }
    mrow[h] = m;
    wgt[h] = w;
  }
  float acc[K][W];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < W; ++e) acc[k][e] = 0.f;
  const int base = threadIdx.x & 32;   // first lane of this half wave within the wave
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    for (int c = 0; c < 32; ++c) {
      const int m = __shfl(mrow[h], base + c);
      if (m < 0) continue;             // uniform over the half wave
      const float w = __shfl(wgt[h], base + c);
      const float* r = rows + (int64_t)m * C;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int ch = (k * kLanes + lane) * W;
        if (ch < C) {
          float rv[W];
          load_w<W>(r + ch, rv);
#pragma unroll
          for (int e = 0; e < W; ++e) acc[k][e] += w * rv[e];
        }
      }
    }
  }
  float* out = grad + j * C;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = (k * kLanes + lane) * W;
    if (ch < C) store_w<W>(out + ch, acc[k]);
  }
}

inline unsigned groups(int64_t n) { return (unsigned)((n + kPerWG - 1) / kPerWG); }

// chunks of 32 * W channels that hold C: the instantiated counts
inline int chunks(int C, int W) {
  const int k = (C + 32 * W - 1) / (32 * W);
  if (W == 4) return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 6 ? 6 : 8;
  return k <= 1 ? 1 : k <= 4 ? 4 : 32;
}

// call `fn<W, K>()` for the instantiated (W, K) that holds C channels
#define VEON_ALIGN_DISPATCH(vec, C, CALL)                       \
  do {                                                          \
    if (vec) {                                                  \
      switch (chunks(C, 4)) {                                   \
        case 1: CALL(4, 1); break;                              \
        case 2: CALL(4, 2); break;                              \
        case 4: CALL(4, 4); break;                              \
        case 6: CALL(4, 6); break;                              \
        default: CALL(4, 8); break;                             \
      }                                                         \
    } else {                                                    \
      switch (chunks(C, 1)) {                                   \
        case 1: CALL(1, 1); break;                              \
        case 4: CALL(1, 4); break;                              \
        default: CALL(1, 32); break;                            \
      }                                                         \
    }                                                           \
  } while (0)

struct Common {
  Strides5 fs;
  Grid g;
  const float* fb;
  bool vec;
};

// shared argument checks of the two entry points; false = VEON_ERR_BAD_ARG
bool common_args(const float* feat, const int64_t* st, int C, int B, int zi, int yi, int xi,
                 int Zo, int Yo, int Xo, const int* voxels, const int* labels, int N,
                 int batch, const float* table, int K, float eps, Common* out) {
  if (!feat || !st || (N > 0 && (!voxels || !labels)) || !table || C <= 0 || C > kMaxC ||
      K < 1 || N < 0 ||
      B <= 0 || batch < 0 || batch >= B || zi <= 0 || yi <= 0 || xi <= 0 || Zo <= 0 ||
      Yo <= 0 || Xo <= 0 || !(eps > 0.f))
    return false;
  if (!aligned(feat, 4) || !aligned(voxels, 4) || !aligned(labels, 4) || !aligned(table, 4))
    return false;
  if (st[0] < 0 || st[1] <= 0 || st[2] < 0 || st[3] < 0 || st[4] < 0) return false;
  // channels-last rows: C may not run past the row into the next voxel
  if (st[1] == 1 && xi > 1 && C > st[4]) return false;
  out->fs = strides5(st);
  out->g = Grid{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
                (float)xi / (float)Xo};
  out->fb = feat + batch * st[0];
  out->vec = st[1] == 1 && C % 4 == 0 && aligned(out->fb, 16) && aligned(table, 16) &&
             st[2] % 4 == 0 && st[3] % 4 == 0 && st[4] % 4 == 0;
  return true;
}

}  // namespace

extern "C" int veon_occ_align_fwd(const float* feat, const int64_t* feat_strides, int C, int B,
                                  int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                  const int* voxels, const int* labels, int N, int batch,
                                  const float* table, int K, float eps, float* table_norms,
                                  float* cos_out, float* stats, void* stream) {
  Common c;
  if (!common_args(feat, feat_strides, C, B, zi, yi, xi, Zo, Yo, Xo, voxels, labels, N, batch,
                   table, K, eps, &c) ||
      !table_norms || !aligned(table_norms, 4) ||
      (N > 0 && (!cos_out || !stats || !aligned(cos_out, 4) || !aligned(stats, 4))))
    return VEON_ERR_BAD_ARG;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_table_norms, dim3((unsigned)K), dim3(64), 0, s, table, C, eps,
                     table_norms);
  if (N == 0) return launch_status();
#define CALL(W, KK)                                                                          \
  hipLaunchKernelGGL((k_align_fwd<W, KK>), dim3(groups(N)), dim3(256), 0, s, c.fb, c.fs, C,  \
                     c.g, voxels, labels, N, table, table_norms, K, eps, cos_out, stats)
  VEON_ALIGN_DISPATCH(c.vec, C, CALL);
#undef CALL
  return launch_status();
}

extern "C" int veon_occ_align_bwd(const float* feat, const int64_t* feat_strides, int C, int B,
                                  int zi, int yi, int xi, const int* voxels, const int* labels,
                                  int N, int batch, const float* table, int K, float eps,
                                  const float* table_norms, const float* stats, const float* g,
                                  const int* order, const int* seg_start, int M,
                                  const int* occ_rows, float* rows, float* grad, void* stream) {
  Common c;
  if (zi <= 0 || yi <= 0 || xi <= 0 || zi > (1 << 20) || yi > (1 << 20) || xi > (1 << 20) ||
      !common_args(feat, feat_strides, C, B, zi, yi, xi, 2 * zi, 2 * yi, 2 * xi, voxels,
                   labels, N, batch, table, K, eps, &c) ||
      !grad || !aligned(grad, 4) || !occ_rows || !aligned(occ_rows, 4) || M < 0 || M > N ||
      (M > 0 && (!table_norms || !stats || !g || !order || !seg_start || !rows ||
                 !aligned(table_norms, 4) || !aligned(stats, 4) || !aligned(g, 4) ||
                 !aligned(order, 4) || !aligned(seg_start, 4) || !aligned(rows, 4))))
    return VEON_ERR_BAD_ARG;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (M > 0) {
    const bool vec = c.vec && aligned(rows, 16);
#define CALL(W, KK)                                                                           \
  hipLaunchKernelGGL((k_align_rows<W, KK>), dim3(groups(M)), dim3(256), 0, s, c.fb, c.fs, C,  \
                     c.g, voxels, labels, N, table, table_norms, K, eps, stats, g, order,     \
                     seg_start, M, rows)
    VEON_ALIGN_DISPATCH(vec, C, CALL);
#undef CALL
  }
  const bool vec_b = C % 4 == 0 && aligned(grad, 16) && (M == 0 || aligned(rows, 16));
  const int64_t nlow = (int64_t)zi * yi * xi;
#define CALL(W, KK)                                                                        \
  hipLaunchKernelGGL((k_align_gather<W, KK>), dim3(groups(nlow)), dim3(256), 0, s, rows, M, \
                     occ_rows, C, c.g, grad)
  VEON_ALIGN_DISPATCH(vec_b, C, CALL);
#undef CALL
  return launch_status();
}
