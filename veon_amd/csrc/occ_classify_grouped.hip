// The occupancy tail against a DETAILED vocabulary (SANInVeonTemporal._merge_classes_prob,
// san_in_veon_entry_temporal.py:273-297, + VEONTemporal.simple_test, veon_temporal.py:
// 220-229): the classifier scores K = K2 + 1 rows ("car", "sedan", "hatch-back", ... and
// the background row), every run of rows that describes one class is merged by its
// maximum, and the label is the arg-max over the n_merged merged channels.  The reference
// upsamples all K rows first (150 MB of fp32 at 200 x 200 x 16 for some 60 rows); here the
// K upsampled rows exist only in registers:
//
//   k_occ_labels_grouped    the uint8 label volume and nothing else, optionally with the
//                           confusion matrix: k_occ_labels (occ_eval.hip) with the merge
//                           in its class loop -- the same tile walk (occ_label_tile.h)
//   k_occ_classify_grouped  int64 labels, the upsampled occupancy pair and the MERGED
//                           logits: k_occ_classify (occ_head.hip) likewise; a merged
//                           channel is stored once, when its run ends
//
// Both blend every row with occ_interp.h (`source`, `corner_offsets`, `blend`), so a row's
// upsampled value is bit-equal to k_occ_classify's.  The group table travels in the kernel
// arguments (256 bytes) and is copied to LDS once per block; a class loop reads it with
// wave-uniform addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occ_interp.h"
#include "occ_label_tile.h"

namespace {

constexpr int MAX_ROWS = 256;
constexpr int MAX_MERGED = 64;
constexpr unsigned RUN_ENDS = 0x80u;

// entry c: the merged channel of row c, | RUN_ENDS on the last row of its run; zero past K
struct GroupTable {
  uint8_t e[MAX_ROWS];
};

// One output voxel: the label; with STORE also the merged logits to so[channel * plane];
// the upsampled occupancy logits to o[0..1].  tab: the group table in LDS.
template <bool VEC4, bool STORE>
__device__ __forceinline__ int grouped_voxel(
    const float* __restrict__ sem, const Strides5& ss, int K, const uint8_t* tab,
    int free_label, const float* __restrict__ bin, const Strides5& bs, const Axis& az,
    const Axis& ay, const Axis& ax, int b, float* __restrict__ so, int64_t plane, float* o) {
  float vmax = -INFINITY;    // best merged value and the lowest channel that attains it
  int cls = MAX_ROWS;
  float run = -INFINITY;     // maximum of the current run, NaN once a row of it is NaN
  bool bad = false;
  const float* sp = sem + b * ss.b;
  int ks[8];
  corner_offsets(ks, ss, az, ay, ax);
  auto row = [&](unsigned entry, float val) {
    bad |= val != val;
    run = run != run ? run : ((val != val || val > run) ? val : run);
    if (entry & RUN_ENDS) {
      const int chan = (int)(entry & (RUN_ENDS - 1u));
      if (STORE) so[(int64_t)chan * plane] = run;
      if (run > vmax || (run == vmax && chan < cls)) {
        vmax = run;
        cls = chan;
      }
      run = -INFINITY;
    }
  };
  if (VEC4) {
#pragma unroll 1
    for (int c = 0; c < K; c += 4) {
      float4 k4[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) k4[q] = *reinterpret_cast<const float4*>(sp + c + ks[q]);
      const unsigned entries = *reinterpret_cast<const unsigned*>(tab + c);
      float val4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float k8[8];   // row c + e of the eight corners
#pragma unroll
        for (int q = 0; q < 8; ++q) k8[q] = reinterpret_cast<const float*>(&k4[q])[e];
        val4[e] = blend(k8, az, ay, ax);
      }
      // (as in k_occ_labels: keeps the 16-byte corner loads whole)
#pragma unroll
      for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(val4[e]));
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < K) row((entries >> (8 * e)) & 0xffu, val4[e]);
    }
  } else {
#pragma unroll 2
    for (int c = 0; c < K; ++c) row(tab[c], blend(sp + c * ss.c, ks, az, ay, ax));
  }
  const bool scored = !bad && vmax < INFINITY && vmax > -INFINITY;
  const float* bp = bin + b * bs.b;
  int kb[8];
  corner_offsets(kb, bs, az, ay, ax);
  const float o0 = blend(bp, kb, az, ay, ax), o1 = blend(bp + bs.c, kb, az, ay, ax);
  o[0] = o0;
  o[1] = o1;
  const float om = o0 > o1 ? o0 : o1;
  const float e0 = expf(o0 - om), e1 = expf(o1 - om);
  const bool keep = scored && (e0 / (e0 + e1) > 0.5f);
  return keep ? cls : free_label;
}

// the block's copy of the table; THREADS == MAX_ROWS: one byte per lane
__device__ __forceinline__ void stage_table(uint8_t* tab, const GroupTable& table) {
  static_assert(THREADS == MAX_ROWS, "one table byte per lane");
  tab[threadIdx.x] = table.e[threadIdx.x];
  __syncthreads();
}

template <bool VEC4, int W>
__global__ __launch_bounds__(THREADS) void k_occ_labels_grouped(
    const float* __restrict__ sem, Strides5 ss, int K, GroupTable table, int n_cl,
    int free_label, const float* __restrict__ bin, Strides5 bs, int B, Geometry g, int TY,
    uint8_t* __restrict__ labels, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, unsigned long long* __restrict__ hist) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint8_t* tab = smem;   // MAX_ROWS bytes, then the tile walk's
  stage_table(tab, table);
  label_tiles<W>(
      smem + MAX_ROWS,
      [&](int b, int z, int y, int x) {
        const Axis az = source(z, g.scz, g.zi), ay = source(y, g.scy, g.yi),
                   ax = source(x, g.scx, g.xi);
        float o[2];
        return grouped_voxel<VEC4, false>(sem, ss, K, tab, free_label, bin, bs, az, ay, ax,
                                          b, nullptr, 0, o);
      },
      n_cl, B, g, TY, labels, gt, mask, hist);
}

// one lane = one output voxel, x fastest, as k_occ_classify
template <bool VEC4>
__global__ __launch_bounds__(THREADS) void k_occ_classify_grouped(
    const float* __restrict__ sem, Strides5 ss, int K, GroupTable table, int n_merged,
    int free_label, const float* __restrict__ bin, Strides5 bs, int B, Geometry g,
    float* __restrict__ merged_out, float* __restrict__ bin_out,
    int64_t* __restrict__ cls_out) {
  __shared__ __align__(16) uint8_t tab[MAX_ROWS];
  stage_table(tab, table);
  // 32-bit index arithmetic (the host checks B*Zo*Yo*Xo < 2^31)
  const unsigned idx = blockIdx.x * (unsigned)THREADS + threadIdx.x;
  const unsigned plane32 = (unsigned)g.Zo * g.Yo * g.Xo;
  if (idx >= (unsigned)B * plane32) return;
  const int b = (int)(idx / plane32);
  const unsigned v = idx - (unsigned)b * plane32;
  const int x = (int)(v % (unsigned)g.Xo);
  const int y = (int)((v / (unsigned)g.Xo) % (unsigned)g.Yo);
  const int z = (int)(v / ((unsigned)g.Xo * g.Yo));
  const int64_t plane = plane32;
  const Axis az = source(z, g.scz, g.zi), ay = source(y, g.scy, g.yi),
             ax = source(x, g.scx, g.xi);
  float o[2];
  const int label = grouped_voxel<VEC4, true>(
      sem, ss, K, tab, free_label, bin, bs, az, ay, ax, b,
      merged_out + (int64_t)b * n_merged * plane + v, plane, o);
  bin_out[((int64_t)b * 2 + 0) * plane + v] = o[0];
  bin_out[((int64_t)b * 2 + 1) * plane + v] = o[1];
  cls_out[(((int64_t)b * g.Xo + x) * g.Yo + y) * g.Zo + z] = label;
}

// group (HOST, K bytes) -> the kernels' table; false unless every row's channel is below
// n_merged, the rows of a channel are consecutive and every channel has exactly one run
bool make_table(const uint8_t* group, int K, int n_merged, GroupTable* table) {
  bool used[MAX_MERGED] = {};
  int runs = 0;
  for (int c = 0; c < MAX_ROWS; ++c) table->e[c] = 0;
  for (int c = 0; c < K; ++c) {
    if (group[c] >= n_merged) return false;
    const bool ends = c + 1 == K || group[c + 1] != group[c];
    table->e[c] = (uint8_t)(group[c] | (ends ? RUN_ENDS : 0u));
    if (ends) {
      if (used[group[c]]) return false;
      used[group[c]] = true;
      ++runs;
    }
  }
  return runs == n_merged;
}

bool common_args_ok(const float* sem, const int64_t* sem_strides, int K,
                    const uint8_t* group, int n_merged, int free_label, const float* bin,
                    const int64_t* bin_strides, int B, int zi, int yi, int xi, int Zo, int Yo,
                    int Xo) {
  if (!sem || !bin || !sem_strides || !bin_strides || !group || K <= 0 || K > MAX_ROWS ||
      n_merged <= 0 || n_merged > MAX_MERGED || free_label < 0 || free_label > 255 ||
      B <= 0 || zi <= 0 || yi <= 0 || xi <= 0 || Zo <= 0 || Yo <= 0 || Xo <= 0)
    return false;
  if ((int64_t)B * Zo * Yo * Xo > 0x7fffffffLL) return false;
  return strides_fit(sem_strides, zi, yi, xi) && strides_fit(bin_strides, zi, yi, xi);
}

Geometry geometry(int zi, int yi, int xi, int Zo, int Yo, int Xo) {
  // ATen: scale = in / out in float (area_pixel_compute_scale, no scale_factor given)
  return Geometry{zi, yi, xi, Zo, Yo, Xo, (float)zi / (float)Zo, (float)yi / (float)Yo,
                  (float)xi / (float)Xo};
}

template <bool VEC4>
void launch_labels_grouped(const TileLaunch& t, size_t lds, hipStream_t st, const float* sem,
                           const Strides5& ss, int K, const GroupTable& table, int n_cl,
                           int free_label, const float* bin, const Strides5& bs, int B,
                           const Geometry& g, uint8_t* labels, const uint8_t* gt,
                           const uint8_t* mask, unsigned long long* hist) {
#define VEON_LABELS(w)                                                                     \
  hipLaunchKernelGGL((k_occ_labels_grouped<VEC4, w>), dim3((unsigned)t.blocks),            \
                     dim3(THREADS), lds, st, sem, ss, K, table, n_cl, free_label, bin, bs, \
                     B, g, t.TY, labels, gt, mask, hist)
  switch (t.W) {
    case 16: VEON_LABELS(16); break;
    case 8: VEON_LABELS(8); break;
    case 4: VEON_LABELS(4); break;
    default: VEON_LABELS(1); break;
  }
#undef VEON_LABELS
}

}  // namespace

extern "C" int veon_occ_labels_grouped(const float* sem, const int64_t* sem_strides, int K,
                                       const uint8_t* group, int n_merged, int free_label,
                                       const float* bin, const int64_t* bin_strides, int B,
                                       int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                       uint8_t* labels, const uint8_t* gt,
                                       const uint8_t* mask, int64_t* hist, void* stream) {
  if (!labels || Zo > MAX_ZO ||
      !common_args_ok(sem, sem_strides, K, group, n_merged, free_label, bin, bin_strides, B,
                      zi, yi, xi, Zo, Yo, Xo))
    return VEON_ERR_BAD_ARG;
  // the histogram needs the ground truth and the other way round; a mask needs both
  if ((gt != nullptr) != (hist != nullptr) || (mask && !gt)) return VEON_ERR_BAD_ARG;
  const int n_cl = n_merged > free_label + 1 ? n_merged : free_label + 1;
  if (hist && n_cl > MAX_CL) return VEON_ERR_BAD_ARG;
  GroupTable table;
  if (!make_table(group, K, n_merged, &table)) return VEON_ERR_BAD_ARG;
  const Strides5 ss = strides5(sem_strides), bs = strides5(bin_strides);
  const Geometry g = geometry(zi, yi, xi, Zo, Yo, Xo);
  const TileLaunch t = tile_launch(B, Zo, Yo, Xo, n_cl, labels, gt, mask, hist != nullptr);
  const size_t lds = MAX_ROWS + t.lds;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  if (vec4_rows(sem, ss, K))
    launch_labels_grouped<true>(t, lds, st, sem, ss, K, table, n_cl, free_label, bin, bs, B,
                                g, labels, gt, mask, h);
  else
    launch_labels_grouped<false>(t, lds, st, sem, ss, K, table, n_cl, free_label, bin, bs, B,
                                 g, labels, gt, mask, h);
  return launch_status();
}

extern "C" int veon_occ_classify_grouped(const float* sem, const int64_t* sem_strides, int K,
                                         const uint8_t* group, int n_merged, int free_label,
                                         const float* bin, const int64_t* bin_strides, int B,
                                         int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                         float* merged_out, float* bin_out, int64_t* cls_out,
                                         void* stream) {
  if (!merged_out || !bin_out || !cls_out ||
      !common_args_ok(sem, sem_strides, K, group, n_merged, free_label, bin, bin_strides, B,
                      zi, yi, xi, Zo, Yo, Xo))
    return VEON_ERR_BAD_ARG;
  GroupTable table;
  if (!make_table(group, K, n_merged, &table)) return VEON_ERR_BAD_ARG;
  const Strides5 ss = strides5(sem_strides), bs = strides5(bin_strides);
  const Geometry g = geometry(zi, yi, xi, Zo, Yo, Xo);
  const int64_t blocks = ((int64_t)B * Zo * Yo * Xo + THREADS - 1) / THREADS;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec4_rows(sem, ss, K))
    hipLaunchKernelGGL(k_occ_classify_grouped<true>, dim3((unsigned)blocks), dim3(THREADS), 0,
                       st, sem, ss, K, table, n_merged, free_label, bin, bs, B, g, merged_out,
                       bin_out, cls_out);
  else
    hipLaunchKernelGGL(k_occ_classify_grouped<false>, dim3((unsigned)blocks), dim3(THREADS),
                       0, st, sem, ss, K, table, n_merged, free_label, bin, bs, B, g,
                       merged_out, bin_out, cls_out);
  return launch_status();
}
