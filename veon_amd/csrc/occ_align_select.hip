// The discrete half of VEON's 2D->3D feature-alignment loss (Proj2Dto3DLoss,
// models/semantic_net/loss/occ_loss_utils/occ3d_nuscenes.py:372-508): which (camera, voxel)
// pairs of one sample the loss trains on, with which label and which weight.  The torch
// formulation is several dozen launches with about ten host synchronisations (nonzero,
// boolean-mask gathers, tolist, bincount); here it is seven kernels in three entry points,
// and the host reads back two small tensors (the kept count, which sizes the lists, and
// the final counts).
//
//   mark      one lane per (camera, voxel) pair, camera-major, voxels in the label
//             tensor's own order: label test, projection, the six in-view comparisons;
//             one 64-bit ballot per wave and one kept total per workgroup
//   scan      one workgroup walks the totals in passes of 1024 with a carry
//   compact   one lane per pair: a kept pair stores its index at offset + rank
//   classify  one lane per KEPT entry: bilinear sample of the K2 logits, the three
//             arg-maxes (streamed over the classes, nothing indexed in registers)
//   count     stage-2 drop flag from the retrieval scores, final det / soft flags,
//             integer histograms per (term, camera, class) (LDS first, then one global
//             integer atomic per non-empty bin: the result does not depend on order)
//   scan + finish + emit   positions of the det and of the soft entries, the per-camera
//             normalisers, and the lists: det entries first, then soft, in kept order
//
// The ORDER of every list comes from the scans, never from an atomic ticket, and no float
// is ever added atomically: repeated calls are bit-identical.
// No half operands: the file is identical in both library flavours.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_common.h"

namespace {

constexpr int kWG = 256;         // lanes per workgroup of the per-pair / per-entry kernels
constexpr int kWaves = kWG / 64;
constexpr int kScan = 1024;      // totals one pass of the scan workgroup takes
constexpr int kMaxCam = 32;      // cameras the histogram in LDS holds
constexpr int kMaxCls = 32;      // merged classes (VEON: 17)
constexpr int kCamFloats = 24;   // ego2img rows 0-2 (3 x 4), post_rots (3 x 3), post_trans

struct Geom {
  int n_cam, Xo, Yo, Zo;
  int n_vox;                     // Xo * Yo * Zo
  float sx, ox, sy, oy, sz, oz;  // centre = i * step + offset, offset = lo + step / 2
  float umax, vmax;              // image width - 1, height - 1
  float dlo, dhi;
};

// Voxel centre -> (u, v, depth) in the augmented image, the mirror's operation sequence:
// the 3 x 4 affine, x and y over z, the full 3 x 3 post rotation plus the translation.
// -> the six in-view comparisons (false for NaN, as in torch).
__device__ __forceinline__ bool project(const float* __restrict__ m, const Geom& g, int vox,
                                        float& u, float& v) {
  const int yz = g.Yo * g.Zo;
  const int xi = vox / yz, r = vox - xi * yz;
  const int yi = r / g.Zo, zi = r - yi * g.Zo;
  const float x = (float)xi * g.sx + g.ox, y = (float)yi * g.sy + g.oy,
              z = (float)zi * g.sz + g.oz;
  const float px = x * m[0] + y * m[1] + z * m[2] + m[3];
  const float py = x * m[4] + y * m[5] + z * m[6] + m[7];
  const float pz = x * m[8] + y * m[9] + z * m[10] + m[11];
  const float a = px / pz, b = py / pz;
  u = a * m[12] + b * m[13] + pz * m[14] + m[21];
  v = a * m[15] + b * m[16] + pz * m[17] + m[22];
  const float d = a * m[18] + b * m[19] + pz * m[20] + m[23];
  return u >= 0.f && u <= g.umax && v >= 0.f && v <= g.vmax && d < g.dhi && d >= g.dlo;
}

__device__ __forceinline__ int load_label(const void* labels, int is64, int vox) {
  if (is64) {
    const long long l = static_cast<const long long*>(labels)[vox];
    return l < 0 || l > 255 ? -1 : (int)l;
  }
  return static_cast<const unsigned char*>(labels)[vox];
}

__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
  const unsigned lane = threadIdx.x & 63u;
  return __popcll(mask & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kWG) void k_mark(const void* __restrict__ labels, int is64,
                                              int n_cls, const float* __restrict__ cams, Geom g,
                                              int n_pairs, unsigned long long* __restrict__ masks,
                                              int* __restrict__ totals) {
  __shared__ int cnt[kWaves];
  const int p = blockIdx.x * kWG + threadIdx.x;   // n_pairs + kWG < 2^31 (checked on the host)
  bool keep = false;
  if (p < n_pairs) {
    const int cam = p / g.n_vox, vox = p - cam * g.n_vox;
    const int lab = load_label(labels, is64, vox);
    if (lab >= 0 && lab < n_cls) {
      float u, v;
      keep = project(cams + cam * kCamFloats, g, vox, u, v);
    }
  }
  const unsigned long long mask = __ballot(keep);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    masks[(int64_t)blockIdx.x * kWaves + wave] = mask;
    cnt[wave] = __popcll(mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) totals[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// Exclusive scan in place of `rows` arrays of n ints (one workgroup per row, passes of
// kScan with a carry); sums[row] = the row's total.  Row 0 also clears `zero`.
__global__ __launch_bounds__(kScan) void k_scan(int* __restrict__ data, int n,
                                                int* __restrict__ sums, int* __restrict__ zero,
                                                int n_zero) {
  __shared__ int wsum[kScan / 64];
  int* d = data + (int64_t)blockIdx.x * n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kScan) {
    const int i = base + threadIdx.x;
    const int v = i < n ? d[i] : 0;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScan / 64; ++w) {
      const int s = wsum[w];
      if (w < wave) before += s;
      total += s;
    }
    if (i < n) d[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = carry;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < n_zero; i += kScan) zero[i] = 0;
}

// A kept pair stores its index at its position; the lane of the last camera's first pair
// stores that position (kept or not: the number of entries in front of the camera).
__global__ __launch_bounds__(kWG) void k_compact(const unsigned long long* __restrict__ masks,
                                                 const int* __restrict__ offsets, int n_pairs,
                                                 int last_cam_pair, int cap,
                                                 int* __restrict__ pair, int* __restrict__ first_last) {
  const int p = blockIdx.x * kWG + threadIdx.x;
  const int wave = threadIdx.x >> 6;
  const unsigned long long* wm = masks + (int64_t)blockIdx.x * kWaves;
  int pos = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos += __popcll(wm[w]);
  const unsigned long long mask = wm[wave];
  pos += lanes_below(mask);
  if (p == last_cam_pair) *first_last = pos;
  if (p < n_pairs && ((mask >> (threadIdx.x & 63)) & 1ull) && pos < cap) pair[pos] = p;
}

__device__ __forceinline__ float texel(const float* __restrict__ plane, int y, int x, int hs,
                                       int ws) {
  return (x >= 0 && x < ws && y >= 0 && y < hs) ? plane[y * ws + x] : 0.f;
}

// flags: bit 0 det, bit 1 soft
__global__ __launch_bounds__(kWG) void k_classify(
    const void* __restrict__ labels, int is64, const float* __restrict__ cams, Geom g,
    const float* __restrict__ sem, int K2, int hs, int ws, float half_w, float half_h,
    const int* __restrict__ gid, int open_from, const int* __restrict__ pair, int n,
    const int* __restrict__ first_last, int is_last, int* __restrict__ vox3,
    int4* __restrict__ cls, int* __restrict__ flags) {
  const int i = blockIdx.x * kWG + threadIdx.x;
  if (i >= n) return;
  const int p = pair[i];
  if (p < 0 || p >= g.n_cam * g.n_vox) {   // n does not belong to these masks: reads nothing
    cls[i] = make_int4(0, 0, 0, 0);
    flags[i] = 0;
    return;
  }
  const int cam = p / g.n_vox, vox = p - cam * g.n_vox;
  const int gt = load_label(labels, is64, vox);
  float u, v;
  project(cams + cam * kCamFloats, g, vox, u, v);
  // F.grid_sample(bilinear, align_corners=False, zeros) on the map's own size
  const float gx = u / half_w - 1.f, gy = v / half_h - 1.f;
  const float ix = ((gx + 1.f) * (float)ws - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)hs - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float w_nw = (fx + 1.f - ix) * (fy + 1.f - iy), w_ne = (ix - fx) * (fy + 1.f - iy);
  const float w_sw = (fx + 1.f - ix) * (iy - fy), w_se = (ix - fx) * (iy - fy);
  const float* plane = sem + (int64_t)cam * K2 * hs * ws;

  const float ninf = -__builtin_huge_valf();
  float best = ninf, gbest = ninf, mbest = ninf, rbest = ninf;
  int plain = 0, merged = 0, restricted = 0, group = 0;
  for (int k = 0; k < K2; ++k, plane += hs * ws) {
    float val = 0.f;
    val += texel(plane, y0, x0, hs, ws) * w_nw;
    val += texel(plane, y0, x0 + 1, hs, ws) * w_ne;
    val += texel(plane, y0 + 1, x0, hs, ws) * w_sw;
    val += texel(plane, y0 + 1, x0 + 1, hs, ws) * w_se;
    const int gk = gid[k];
    if (val > best) { best = val; plain = k; }
    if (gk == gt && val > rbest) { rbest = val; restricted = k; }
    if (gk != group) {                     // the groups are runs of consecutive classes
      if (gbest > mbest) { mbest = gbest; merged = group; }
      group = gk;
      gbest = ninf;
    }
    gbest = fmaxf(gbest, val);
  }
  if (gbest > mbest) merged = group;

  bool soft = merged == gt || gt >= open_from;
  bool det = !soft;
  if (is_last && i == *first_last) soft = det = true;    // the reference's forced entry
  const int yz = g.Yo * g.Zo;
  const int xi = vox / yz, r = vox - xi * yz;
  vox3[3 * i] = xi;
  vox3[3 * i + 1] = r / g.Zo;
  vox3[3 * i + 2] = r % g.Zo;
  cls[i] = make_int4(gt, plain, merged, restricted);
  flags[i] = (det ? 1 : 0) | (soft ? 2 : 0);
}

// Final flags (stage 2 when `score` is given), histograms, per-workgroup det / soft totals.
// hist: [2][n_cam][n_cls] then ignored [n_cam]; totals: [2][n_wg].
__global__ __launch_bounds__(kWG) void k_count(
    const int* __restrict__ pair, const int4* __restrict__ cls, int* __restrict__ flags, int n,
    int n_vox, int n_cam, int n_cls, const float* __restrict__ score,
    const float* __restrict__ tnorm, int K2, const int* __restrict__ gid, float thr,
    const float* __restrict__ priority, int* __restrict__ hist, int* __restrict__ totals) {
  __shared__ int bins[2 * kMaxCam * kMaxCls + kMaxCam];
  __shared__ int cnt[2][kWaves];
  const int n_bins = 2 * n_cam * n_cls + n_cam;
  for (int b = threadIdx.x; b < n_bins; b += kWG) bins[b] = 0;
  __syncthreads();
  const int i = blockIdx.x * kWG + threadIdx.x;
  bool det = false, soft = false;
  if (i < n) {
    const int cam = pair[i] / n_vox;
    const int4 c = cls[i];
    const int f = flags[i];
    det = f & 1;
    soft = f & 2;
    if (score) {
      const float ninf = -__builtin_huge_valf();
      float best = ninf, sbest = 0.f, gbest = ninf, mbest = ninf;
      int pred = 0, group = 0;
      for (int k = 0; k < K2; ++k) {
        const float s = score[(int64_t)k * n + i];
        const float dot = s * tnorm[k];            // ranks the classes as <f, t_k> does
        if (dot > best) { best = dot; sbest = s; }
        const int gk = gid[k];
        if (gk != group) {
          if (gbest > mbest) { mbest = gbest; pred = group; }
          group = gk;
          gbest = ninf;
        }
        gbest = fmaxf(gbest, dot);
      }
      if (gbest > mbest) pred = group;
      if (best == ninf) sbest = score[i];          // arg-max 0 when nothing compares greater
      const bool drop = sbest >= thr && priority[pred] > priority[c.z];
      if (soft && drop) {
        atomicAdd(&bins[2 * n_cam * n_cls + cam], 1);
        soft = false;
      }
    }
    flags[i] = (det ? 1 : 0) | (soft ? 2 : 0);
    if (det) atomicAdd(&bins[cam * n_cls + c.x], 1);
    if (soft) atomicAdd(&bins[(n_cam + cam) * n_cls + c.z], 1);
  }
  const unsigned long long md = __ballot(det), ms = __ballot(soft);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    cnt[0][wave] = __popcll(md);
    cnt[1][wave] = __popcll(ms);
  }
  __syncthreads();
  if (threadIdx.x < 2)
    totals[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] =
        cnt[threadIdx.x][0] + cnt[threadIdx.x][1] + cnt[threadIdx.x][2] + cnt[threadIdx.x][3];
  for (int b = threadIdx.x; b < n_bins; b += kWG)
    if (bins[b]) atomicAdd(&hist[b], bins[b]);
}

// Per (term, camera): entries, sum of the priorities of the classes present, share of the
// term's entries.  result: n_det, n_soft, det[n_cam], soft[n_cam], ignored[n_cam].
__global__ __launch_bounds__(64) void k_finish(const int* __restrict__ hist,
                                               const int* __restrict__ sums, int n_cam, int n_cls,
                                               const float* __restrict__ priority,
                                               float* __restrict__ norm, float* __restrict__ ratio,
                                               int* __restrict__ result) {
  __shared__ int per_cam[2 * kMaxCam];
  const int t = threadIdx.x;
  if (t < 2 * n_cam) {
    const int* h = hist + t * n_cls;
    int cnt = 0;
    float nrm = 0.f;
    for (int c = 0; c < n_cls; ++c) {
      cnt += h[c];
      nrm += (h[c] > 0 ? 1.f : 0.f) * priority[c];
    }
    per_cam[t] = cnt;
    norm[t] = nrm;
    result[2 + t] = cnt;
  }
  if (t < n_cam) result[2 + 2 * n_cam + t] = hist[2 * n_cam * n_cls + t];
  if (t < 2) result[t] = sums[t];
  __syncthreads();
  if (t < 2 * n_cam) {
    const int term = t / n_cam;
    int total = 0;
    for (int c = 0; c < n_cam; ++c) total += per_cam[term * n_cam + c];
    ratio[t] = (float)per_cam[t] / (float)(total < 1 ? 1 : total);
  }
}

__global__ __launch_bounds__(kWG) void k_emit(
    const int* __restrict__ pair, const int* __restrict__ vox3, const int4* __restrict__ cls,
    const int* __restrict__ flags, int n, int n_vox, int n_cam, int n_cls,
    const int* __restrict__ offsets, const int* __restrict__ sums, const int* __restrict__ hist,
    const float* __restrict__ norm, const float* __restrict__ ratio,
    const float* __restrict__ priority, float det_scale, float batch_size, int cap,
    int* __restrict__ out_vox, int* __restrict__ out_lab, float* __restrict__ out_w) {
  __shared__ int cnt[2][kWaves];
  const int i = blockIdx.x * kWG + threadIdx.x;
  const int f = i < n ? flags[i] : 0;
  const unsigned long long md = __ballot(f & 1), ms = __ballot(f & 2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    cnt[0][wave] = __popcll(md);
    cnt[1][wave] = __popcll(ms);
  }
  __syncthreads();
  if (!f) return;
  const int cam = pair[i] / n_vox;
  const int4 c = cls[i];
  const int x = vox3[3 * i], y = vox3[3 * i + 1], z = vox3[3 * i + 2];
#pragma unroll
  for (int term = 0; term < 2; ++term) {
    if (!(f & (1 << term))) continue;
    int pos = offsets[(int64_t)term * gridDim.x + blockIdx.x] + (term ? sums[0] : 0);
    for (int w = 0; w < wave; ++w) pos += cnt[term][w];
    pos += lanes_below(term ? ms : md);
    if (pos >= cap) continue;
    const int klass = term ? c.z : c.x;
    const int tc = term * n_cam + cam;
    float w = 1.f / (float)hist[tc * n_cls + klass];
    if (term) w = w * priority[klass];
    w = w / norm[tc] * ratio[tc];
    if (!term) w = w * det_scale;
    out_vox[3 * pos] = x;
    out_vox[3 * pos + 1] = y;
    out_vox[3 * pos + 2] = z;
    out_lab[pos] = term ? c.y : c.w;
    out_w[pos] = w / batch_size;
  }
}

inline int groups(int64_t n) { return (int)((n + kWG - 1) / kWG); }

bool geom_ok(int n_cam, int Xo, int Yo, int Zo, int n_cls) {
  if (n_cam < 1 || n_cam > kMaxCam || Xo < 1 || Yo < 1 || Zo < 1 || n_cls < 1 ||
      n_cls > kMaxCls)
    return false;
  return (int64_t)n_cam * Xo * Yo * Zo <= (int64_t)INT32_MAX - kWG;
}

Geom make_geom(int n_cam, int Xo, int Yo, int Zo, const float* grid) {
  return Geom{n_cam, Xo, Yo, Zo, Xo * Yo * Zo, grid[0], grid[1], grid[2], grid[3], grid[4],
              grid[5], grid[6], grid[7], grid[8], grid[9]};
}

}  // namespace

extern "C" int64_t veon_align_select_groups(int n_cam, int Xo, int Yo, int Zo) {
  if (!geom_ok(n_cam, Xo, Yo, Zo, 1)) return -1;
  return groups((int64_t)n_cam * Xo * Yo * Zo);
}

extern "C" int veon_align_select_mark(const void* labels, int labels_are_int64, int n_cls,
                                      const float* cams, int n_cam, int Xo, int Yo, int Zo,
                                      const float* grid, unsigned long long* masks,
                                      int* offsets, int* head, int n_head, void* stream) {
  if (!labels || !cams || !grid || !masks || !offsets || !head || n_head < 4 ||
      !geom_ok(n_cam, Xo, Yo, Zo, n_cls) || (labels_are_int64 && !aligned(labels, 8)) ||
      !aligned(cams, 4) || !aligned(masks, 8) || !aligned(offsets, 4) || !aligned(head, 4))
    return VEON_ERR_BAD_ARG;
  const Geom g = make_geom(n_cam, Xo, Yo, Zo, grid);
  const int n_pairs = n_cam * g.n_vox;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_mark, dim3(groups(n_pairs)), dim3(kWG), 0, s, labels, labels_are_int64,
                     n_cls, cams, g, n_pairs, masks, offsets);
  // head[0] = kept entries; head[1..] cleared (head[1]: filled by the compaction)
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScan), 0, s, offsets, groups(n_pairs), head,
                     head + 1, n_head - 1);
  return launch_status();
}

extern "C" int veon_align_select_classify(
    const void* labels, int labels_are_int64, int n_cls, const float* cams, int n_cam, int Xo,
    int Yo, int Zo, const float* grid, const unsigned long long* masks, const int* offsets,
    int* head, const float* sem, int K2, int hs, int ws, float half_w, float half_h,
    const int* gid, int open_from, int n_kept, int is_last, int* pair, int* voxels, int* classes,
    int* flags, void* stream) {
  if (!labels || !cams || !grid || !masks || !offsets || !head || !sem || !gid || !pair ||
      !voxels || !classes || !flags || !geom_ok(n_cam, Xo, Yo, Zo, n_cls) || K2 < 1 ||
      hs < 1 || ws < 1 || (int64_t)n_cam * K2 * hs * ws > INT32_MAX || n_kept < 1 ||
      (int64_t)n_kept > (int64_t)n_cam * Xo * Yo * Zo || !(half_w > 0.f) || !(half_h > 0.f) ||
      (labels_are_int64 && !aligned(labels, 8)) || !aligned(sem, 4) || !aligned(pair, 4) ||
      !aligned(voxels, 4) || !aligned(classes, 16) || !aligned(flags, 4))
    return VEON_ERR_BAD_ARG;
  const Geom g = make_geom(n_cam, Xo, Yo, Zo, grid);
  const int n_pairs = n_cam * g.n_vox;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_compact, dim3(groups(n_pairs)), dim3(kWG), 0, s, masks, offsets, n_pairs,
                     (n_cam - 1) * g.n_vox, n_kept, pair, head + 1);
  hipLaunchKernelGGL(k_classify, dim3(groups(n_kept)), dim3(kWG), 0, s, labels,
                     labels_are_int64, cams, g, sem, K2, hs, ws, half_w, half_h, gid, open_from,
                     pair, n_kept, head + 1, is_last, voxels, reinterpret_cast<int4*>(classes),
                     flags);
  return launch_status();
}

extern "C" int veon_align_select_emit(const int* pair, const int* voxels, const int* classes,
                                      int* flags, int n_kept, int n_cam, int n_vox, int n_cls,
                                      const float* score, const float* table_norms, int K2,
                                      const int* gid, float thr, const float* priority,
                                      float det_scale, int batch_size, int* head, int n_head,
                                      int* totals, float* norms, int* result, int capacity,
                                      int* out_voxels, int* out_labels, float* out_weights,
                                      void* stream) {
  if (!pair || !voxels || !classes || !flags || !gid || !priority || !head || !totals ||
      !norms || !result || !out_voxels || !out_labels || !out_weights || n_kept < 1 ||
      n_cam < 1 || n_cam > kMaxCam || n_cls < 1 || n_cls > kMaxCls || n_vox < 1 || K2 < 1 ||
      batch_size < 1 || capacity < 1 || n_head < 4 + 2 * n_cam * n_cls + n_cam ||
      (score && !table_norms) || !aligned(classes, 16))
    return VEON_ERR_BAD_ARG;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const int wgs = groups(n_kept);
  int* hist = head + 4;
  hipLaunchKernelGGL(k_count, dim3(wgs), dim3(kWG), 0, s, pair,
                     reinterpret_cast<const int4*>(classes), flags, n_kept, n_vox, n_cam, n_cls,
                     score, table_norms, K2, gid, thr, priority, hist, totals);
  hipLaunchKernelGGL(k_scan, dim3(2), dim3(kScan), 0, s, totals, wgs, head + 2,
                     static_cast<int*>(nullptr), 0);
  hipLaunchKernelGGL(k_finish, dim3(1), dim3(64), 0, s, hist, head + 2, n_cam, n_cls, priority,
                     norms, norms + 2 * n_cam, result);
  hipLaunchKernelGGL(k_emit, dim3(wgs), dim3(kWG), 0, s, pair, voxels,
                     reinterpret_cast<const int4*>(classes), flags, n_kept, n_vox, n_cam, n_cls,
                     totals, head + 2, hist, norms, norms + 2 * n_cam, priority, det_scale,
                     (float)batch_size, capacity, out_voxels, out_labels, out_weights);
  return launch_status();
}
