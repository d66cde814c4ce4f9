// Tail of the occupancy path in one pass (SANInVeonTemporal.forward,
// san_in_veon_temporal.py:196-211, and VEONTemporal.simple_test,
// detectors/veon_temporal.py:219-227): trilinear upsampling (align_corners=False)
// of the class logits and of the two occupancy logits from the head's grid to the
// evaluation grid, softmax over the classes -> best class, softmax over
// (occupied, free) -> keep, class-or-free label written in the (X, Y, Z) order of
// the benchmark.  Four kernels, ONE voxel body (`tail_voxel`):
//
//   k_occ_classify          every upsampled class row, the upsampled occupancy pair and
//                           int64 labels.  The reference runs this as ~10 tensor ops over
//                           48 MB of fp32 outputs; here every output element is written
//                           once and nothing else touches HBM (the 6 MB of low-resolution
//                           logits stay in L2): the kernel is bound by its output writes.
//                           One lane = one output voxel, x fastest: every channel plane is
//                           written coalesced; the 8-byte labels go out transposed
//                           (strided), 5 MB in all.
//   k_occ_labels            NOTHING but the uint8 label volume (B,Xo,Yo,Zo) that
//                           VEONTemporal.simple_test returns (veon_temporal.py:219-241):
//                           640 KB at the VEON shape instead of 48 MB of upsampled logits
//                           and 5 MB of int64 labels; optionally the confusion matrix of
//                           Metric_mIoU (occ_metrics.py:78-147) in the same kernel.
//                           Mapping, LDS staging, W-byte output and the histogram's LDS
//                           counters: occ_label_tile.h.
//   k_occ_classify_grouped  against a DETAILED vocabulary (_merge_classes_prob,
//   k_occ_labels_grouped    san_in_veon_entry_temporal.py:273-297, + simple_test,
//                           veon_temporal.py:220-229): the classifier scores K = K2 + 1
//                           rows ("car", "sedan", "hatch-back", ... and the background
//                           row), every run of rows that describes one class is merged by
//                           its maximum, and the label is the arg-max over the n_merged
//                           merged channels (class_runs.h).  The reference upsamples all
//                           K rows first (150 MB of fp32 at 200 x 200 x 16 for some 60
//                           rows); here the K upsampled rows exist only in registers.  The
//                           classify kernel stores a merged channel once, when its run
//                           ends.  The group table travels in the kernel arguments and is
//                           copied to LDS once per block; a class loop reads it with
//                           wave-uniform addresses.
//
// Every kernel blends every row with occ_interp.h (`source`, `corner_offsets`, `blend`) in
// the one body below, so a row's upsampled value, and with it the label, is the same bit
// for bit in all four.
//
// Interpolation follows ATen's upsample_trilinear3d (area_pixel_compute_source_index
// with align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0, the nested
// w/h/t blend); the label is the first maximum of the class logits (= of their
// softmax, up to ties at rounding level).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "class_runs.h"
#include "occ_interp.h"
#include "occ_label_tile.h"

namespace {

// What is done with one row's upsampled value.  A policy has `quad(c)`, called in front of
// the rows c .. c + 3 of a VEC4 step, `row(c, val)`, called for every row in order, and
// afterwards `vmax`, `cls` and `bad`: the best value, its class and "a row was NaN".

// Plain classes: the first maximum; STORE: every row to so[c * plane].
template <bool STORE>
struct PlainRows {
  float* __restrict__ so;
  int64_t plane;
  float vmax = -INFINITY;
  int cls = 0;
  // An int on purpose.  As a bool member the flag was carried through the class loop both as
  // a byte and as a lane mask, and the compiler (ROCm 7.2) did not refresh the lane mask on
  // the paths that skip the surplus rows of the last VEC4 step: a NaN in row K - 1 went
  // unseen for K % 4 of 1 and 2 (the special-value tests catch it).  As a bool local of
  // tail_voxel it was right, and k_occ_classify 5 % slower.
  int bad = 0;
  __device__ __forceinline__ PlainRows(float* so_, int64_t plane_) : so(so_), plane(plane_) {}
  __device__ __forceinline__ void quad(int) {}
  __device__ __forceinline__ void row(int c, float val) {
    if (STORE) so[(int64_t)c * plane] = val;
    bad |= val != val;
    if (val > vmax) {
      vmax = val;
      cls = c;
    }
  }
};

// A detailed vocabulary: the run arg-max fed from the group table in LDS (the four entries
// of a VEC4 step as one 32-bit word, consumed in order); STORE: a merged channel to
// so[channel * plane] when its run ends.
template <bool VEC4, bool STORE>
struct GroupedRows : RunArgMax {
  const uint8_t* tab;
  float* __restrict__ so;
  int64_t plane;
  unsigned entries = 0u;
  __device__ __forceinline__ GroupedRows(const uint8_t* tab_, float* so_, int64_t plane_)
      : tab(tab_), so(so_), plane(plane_) {}
  __device__ __forceinline__ void quad(int c) {
    entries = *reinterpret_cast<const unsigned*>(tab + c);
  }
  __device__ __forceinline__ void row(int c, float val) {
    const unsigned entry = VEC4 ? entries & 0xffu : tab[c];
    if (VEC4) entries >>= 8;
    const int chan = (int)(entry & (RUN_ENDS - 1u));
    const bool ends = (entry & RUN_ENDS) != 0;
    const float merged = RunArgMax::row(chan, ends, val);
    if (STORE && ends) so[(int64_t)chan * plane] = merged;
  }
};

// One output voxel of batch element b at the source positions az, ay, ax: its label, and the
// upsampled occupancy logits in o[0..1].  Every one of the K rows goes to `rows`.
//
// VEC4: the class logits are channels-last (channel stride 1, rows 16-byte aligned,
// at least 4*ceil(K/4) floats per row): four classes per 16-byte corner load -- the
// kernel is bound by the number of cache lines its gathers touch, 3.4x fewer so.
template <bool VEC4, bool PIN, class Rows>
__device__ __forceinline__ int tail_voxel(const float* __restrict__ sem, const Strides5& ss,
                                          int K, Rows& rows, int free_label,
                                          const float* __restrict__ bin, const Strides5& bs,
                                          const Axis& az, const Axis& ay, const Axis& ax,
                                          int b, float* o) {
  // One pass over the classes (a rolled loop: unrolled, the 8 x K corner loads are
  // all hoisted and the kernel drops to one wave per SIMD with scratch).  The best
  // class of softmax(sem) is the first maximum of the logits; its probability
  // 1 / sum(exp(v - vmax)) is positive exactly when the logits hold no NaN and the
  // maximum is finite (otherwise ATen's softmax is NaN and `score > 0` is false).
  const float* sp = sem + b * ss.b;
  int ks[8];
  corner_offsets(ks, ss, az, ay, ax);
  if (VEC4) {
#pragma unroll 1
    for (int c = 0; c < K; c += 4) {
      float4 k4[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) k4[q] = *reinterpret_cast<const float4*>(sp + c + ks[q]);
      rows.quad(c);
      float val4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float k8[8];   // row c + e of the eight corners
#pragma unroll
        for (int q = 0; q < 8; ++q) k8[q] = reinterpret_cast<const float*>(&k4[q])[e];
        val4[e] = blend(k8, az, ay, ax);
      }
      // PIN: every value is needed here, also those of the surplus floats past row K - 1:
      // without the stores of k_occ_classify the compiler otherwise computes them under
      // the branch below, splits each 16-byte load into three and waits for each part.
      if (PIN) {
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(val4[e]));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e < K) rows.row(c + e, val4[e]);
    }
  } else {
#pragma unroll 2
    for (int c = 0; c < K; ++c) rows.row(c, blend(sp + c * ss.c, ks, az, ay, ax));
  }
  const bool scored = !rows.bad && rows.vmax < INFINITY && rows.vmax > -INFINITY;
  const float* bp = bin + b * bs.b;
  int kb[8];
  corner_offsets(kb, bs, az, ay, ax);
  const float o0 = blend(bp, kb, az, ay, ax), o1 = blend(bp + bs.c, kb, az, ay, ax);
  o[0] = o0;
  o[1] = o1;
  const float om = o0 > o1 ? o0 : o1;
  const float e0 = expf(o0 - om), e1 = expf(o1 - om);
  const bool keep = scored && (e0 / (e0 + e1) > 0.5f);
  return keep ? rows.cls : free_label;
}

// The classify kernels: one lane = one output voxel, x fastest.  `make_rows(so, plane)` ->
// the row policy that stores the voxel's n_out channels at so[channel * plane].
template <bool VEC4, bool PIN, class MakeRows>
__device__ __forceinline__ void classify_voxel(
    const float* __restrict__ sem, const Strides5& ss, int K, int n_out, int free_label,
    const float* __restrict__ bin, const Strides5& bs, int B, const Grid& g,
    float* __restrict__ sem_out, float* __restrict__ bin_out, int64_t* __restrict__ cls_out,
    MakeRows make_rows) {
  // 32-bit index arithmetic (the host checks B*Zo*Yo*Xo < 2^31): 64-bit divisions
  // cost ~100 VGPRs here
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
  auto rows = make_rows(sem_out + (int64_t)b * n_out * plane + v, plane);
  float o[2];
  const int label =
      tail_voxel<VEC4, PIN>(sem, ss, K, rows, free_label, bin, bs, az, ay, ax, b, o);
  bin_out[((int64_t)b * 2 + 0) * plane + v] = o[0];
  bin_out[((int64_t)b * 2 + 1) * plane + v] = o[1];
  cls_out[(((int64_t)b * g.Xo + x) * g.Yo + y) * g.Zo + z] = label;
}

// The label kernels: the tile walk with the voxel body as its label; `make_rows()` -> a row
// policy that stores nothing.
template <bool VEC4, int W, class MakeRows>
__device__ __forceinline__ void label_volume(
    unsigned char* smem, const float* __restrict__ sem, const Strides5& ss, int K,
    int free_label, int n_cl, const float* __restrict__ bin, const Strides5& bs, int B,
    const Grid& g, int TY, uint8_t* __restrict__ labels, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, unsigned long long* __restrict__ hist,
    MakeRows make_rows) {
  label_tiles<W>(
      smem,
      [&](int b, int z, int y, int x) {
        const Axis az = source(z, g.scz, g.zi), ay = source(y, g.scy, g.yi),
                   ax = source(x, g.scx, g.xi);
        auto rows = make_rows();
        float o[2];
        return tail_voxel<VEC4, true>(sem, ss, K, rows, free_label, bin, bs, az, ay, ax, b, o);
      },
      n_cl, B, g, TY, labels, gt, mask, hist);
}

// the block's copy of the table; THREADS == MAX_ROWS: one byte per lane
__device__ __forceinline__ void stage_table(uint8_t* tab, const GroupTable& table) {
  static_assert(THREADS == MAX_ROWS, "one table byte per lane");
  tab[threadIdx.x] = table.e[threadIdx.x];
  __syncthreads();
}

template <bool VEC4>
__global__ __launch_bounds__(THREADS) void k_occ_classify(
    const float* __restrict__ sem, Strides5 ss, int Q, const float* __restrict__ bin,
    Strides5 bs, int B, Grid g, float* __restrict__ sem_out, float* __restrict__ bin_out,
    int64_t* __restrict__ cls_out) {
  classify_voxel<VEC4, false>(
      sem, ss, Q, Q, Q, bin, bs, B, g, sem_out, bin_out, cls_out,
      [](float* so, int64_t plane) { return PlainRows<true>(so, plane); });
}

template <bool VEC4>
__global__ __launch_bounds__(THREADS) void k_occ_classify_grouped(
    const float* __restrict__ sem, Strides5 ss, int K, GroupTable table, int n_merged,
    int free_label, const float* __restrict__ bin, Strides5 bs, int B, Grid g,
    float* __restrict__ merged_out, float* __restrict__ bin_out,
    int64_t* __restrict__ cls_out) {
  __shared__ __align__(16) uint8_t tab[MAX_ROWS];
  stage_table(tab, table);
  classify_voxel<VEC4, true>(
      sem, ss, K, n_merged, free_label, bin, bs, B, g, merged_out, bin_out, cls_out,
      [&](float* so, int64_t plane) { return GroupedRows<VEC4, true>(tab, so, plane); });
}

template <bool VEC4, int W>
__global__ __launch_bounds__(THREADS) void k_occ_labels(
    const float* __restrict__ sem, Strides5 ss, int Q, const float* __restrict__ bin,
    Strides5 bs, int B, Grid g, int TY, uint8_t* __restrict__ labels,
    const uint8_t* __restrict__ gt, const uint8_t* __restrict__ mask,
    unsigned long long* __restrict__ hist) {
  extern __shared__ __align__(16) unsigned char smem[];
  label_volume<VEC4, W>(smem, sem, ss, Q, Q, Q + 1, bin, bs, B, g, TY, labels, gt, mask, hist,
                        [] { return PlainRows<false>(nullptr, 0); });
}

template <bool VEC4, int W>
__global__ __launch_bounds__(THREADS) void k_occ_labels_grouped(
    const float* __restrict__ sem, Strides5 ss, int K, GroupTable table, int n_cl,
    int free_label, const float* __restrict__ bin, Strides5 bs, int B, Grid g, int TY,
    uint8_t* __restrict__ labels, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, unsigned long long* __restrict__ hist) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint8_t* tab = smem;   // MAX_ROWS bytes, then the tile walk's
  stage_table(tab, table);
  label_volume<VEC4, W>(smem + MAX_ROWS, sem, ss, K, free_label, n_cl, bin, bs, B, g, TY,
                        labels, gt, mask, hist,
                        [&] { return GroupedRows<VEC4, false>(tab, nullptr, 0); });
}

// ---------------------------------------------------------------------------- host
// What all four entry points check and derive: the volumes, their sizes (the kernels index
// the output with 32 bits) and their strides (32-bit corner offsets).
struct TailArgs {
  Strides5 ss, bs;
  Grid g;
  bool vec4;
};

bool tail_args(const float* sem, const int64_t* sem_strides, int K, const float* bin,
               const int64_t* bin_strides, int B, int zi, int yi, int xi, int Zo, int Yo,
               int Xo, TailArgs* a) {
  if (!sem || !bin || !sem_strides || !bin_strides || K <= 0 || B <= 0 || zi <= 0 ||
      yi <= 0 || xi <= 0 || Zo <= 0 || Yo <= 0 || Xo <= 0)
    return false;
  if ((int64_t)B * Zo * Yo * Xo > 0x7fffffffLL) return false;
  if (!strides_fit(sem_strides, zi, yi, xi) || !strides_fit(bin_strides, zi, yi, xi))
    return false;
  a->ss = strides5(sem_strides), a->bs = strides5(bin_strides);
  a->g = grid_of(zi, yi, xi, Zo, Yo, Xo);
  a->vec4 = vec4_rows(sem, a->ss, K);
  return true;
}

// the label kernels' own: the histogram needs the ground truth and the other way round; a
// mask needs both; n_cl counters a side fit in LDS
bool label_args(const uint8_t* labels, int Zo, const uint8_t* gt, const uint8_t* mask,
                const int64_t* hist, int n_cl) {
  return labels && Zo <= MAX_ZO && (gt != nullptr) == (hist != nullptr) && !(mask && !gt) &&
         !(hist && n_cl > MAX_CL);
}

// the grouped kernels' own: the table of a valid vocabulary
bool group_args(const uint8_t* group, int K, int n_merged, int free_label,
                GroupTable* table) {
  return group && K > 0 && K <= MAX_ROWS && n_merged > 0 && n_merged <= MAX_MERGED &&
         free_label >= 0 && free_label <= 255 && make_table(group, K, n_merged, table);
}

// launch(VEC4 as a std::bool_constant, W of the tile writer as a std::integral_constant)
template <class Launch>
void for_rows_and_width(bool vec4, int W, Launch launch) {
  auto width = [&](auto v4) {
    switch (W) {
      case 16: launch(v4, std::integral_constant<int, 16>{}); break;
      case 8: launch(v4, std::integral_constant<int, 8>{}); break;
      case 4: launch(v4, std::integral_constant<int, 4>{}); break;
      default: launch(v4, std::integral_constant<int, 1>{}); break;
    }
  };
  if (vec4) width(std::true_type{}); else width(std::false_type{});
}

unsigned classify_blocks(int B, const Grid& g) {
  return (unsigned)(((int64_t)B * g.Zo * g.Yo * g.Xo + THREADS - 1) / THREADS);
}

}  // namespace

extern "C" int veon_occ_classify(const float* sem, const int64_t* sem_strides, int Q,
                                 const float* bin, const int64_t* bin_strides, int B,
                                 int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                 float* sem_out, float* bin_out, int64_t* cls_out,
                                 void* stream) {
  TailArgs a;
  if (!sem_out || !bin_out || !cls_out ||
      !tail_args(sem, sem_strides, Q, bin, bin_strides, B, zi, yi, xi, Zo, Yo, Xo, &a))
    return VEON_ERR_BAD_ARG;
  const dim3 blocks(classify_blocks(B, a.g));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.vec4)
    hipLaunchKernelGGL(k_occ_classify<true>, blocks, dim3(THREADS), 0, st, sem, a.ss, Q, bin,
                       a.bs, B, a.g, sem_out, bin_out, cls_out);
  else
    hipLaunchKernelGGL(k_occ_classify<false>, blocks, dim3(THREADS), 0, st, sem, a.ss, Q, bin,
                       a.bs, B, a.g, sem_out, bin_out, cls_out);
  return launch_status();
}

extern "C" int veon_occ_classify_grouped(const float* sem, const int64_t* sem_strides, int K,
                                         const uint8_t* group, int n_merged, int free_label,
                                         const float* bin, const int64_t* bin_strides, int B,
                                         int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                         float* merged_out, float* bin_out, int64_t* cls_out,
                                         void* stream) {
  TailArgs a;
  GroupTable table;
  if (!merged_out || !bin_out || !cls_out ||
      !tail_args(sem, sem_strides, K, bin, bin_strides, B, zi, yi, xi, Zo, Yo, Xo, &a) ||
      !group_args(group, K, n_merged, free_label, &table))
    return VEON_ERR_BAD_ARG;
  const dim3 blocks(classify_blocks(B, a.g));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.vec4)
    hipLaunchKernelGGL(k_occ_classify_grouped<true>, blocks, dim3(THREADS), 0, st, sem, a.ss,
                       K, table, n_merged, free_label, bin, a.bs, B, a.g, merged_out, bin_out,
                       cls_out);
  else
    hipLaunchKernelGGL(k_occ_classify_grouped<false>, blocks, dim3(THREADS), 0, st, sem, a.ss,
                       K, table, n_merged, free_label, bin, a.bs, B, a.g, merged_out, bin_out,
                       cls_out);
  return launch_status();
}

extern "C" int veon_occ_labels(const float* sem, const int64_t* sem_strides, int Q,
                               const float* bin, const int64_t* bin_strides, int B, int zi,
                               int yi, int xi, int Zo, int Yo, int Xo, uint8_t* labels,
                               const uint8_t* gt, const uint8_t* mask, int64_t* hist,
                               void* stream) {
  TailArgs a;
  if (Q > 254 || !label_args(labels, Zo, gt, mask, hist, Q + 1) ||
      !tail_args(sem, sem_strides, Q, bin, bin_strides, B, zi, yi, xi, Zo, Yo, Xo, &a))
    return VEON_ERR_BAD_ARG;
  const TileLaunch t = tile_launch(B, Zo, Yo, Xo, Q + 1, labels, gt, mask, hist != nullptr);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  for_rows_and_width(a.vec4, t.W, [&](auto v4, auto w) {
    hipLaunchKernelGGL((k_occ_labels<decltype(v4)::value, decltype(w)::value>),
                       dim3((unsigned)t.blocks), dim3(THREADS), t.lds, st, sem, a.ss, Q, bin,
                       a.bs, B, a.g, t.TY, labels, gt, mask, h);
  });
  return launch_status();
}

extern "C" int veon_occ_labels_grouped(const float* sem, const int64_t* sem_strides, int K,
                                       const uint8_t* group, int n_merged, int free_label,
                                       const float* bin, const int64_t* bin_strides, int B,
                                       int zi, int yi, int xi, int Zo, int Yo, int Xo,
                                       uint8_t* labels, const uint8_t* gt,
                                       const uint8_t* mask, int64_t* hist, void* stream) {
  TailArgs a;
  GroupTable table;
  if (!tail_args(sem, sem_strides, K, bin, bin_strides, B, zi, yi, xi, Zo, Yo, Xo, &a) ||
      !group_args(group, K, n_merged, free_label, &table))
    return VEON_ERR_BAD_ARG;
  const int n_cl = n_merged > free_label + 1 ? n_merged : free_label + 1;
  if (!label_args(labels, Zo, gt, mask, hist, n_cl)) return VEON_ERR_BAD_ARG;
  const TileLaunch t = tile_launch(B, Zo, Yo, Xo, n_cl, labels, gt, mask, hist != nullptr);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  for_rows_and_width(a.vec4, t.W, [&](auto v4, auto w) {
    hipLaunchKernelGGL((k_occ_labels_grouped<decltype(v4)::value, decltype(w)::value>),
                       dim3((unsigned)t.blocks), dim3(THREADS), MAX_ROWS + t.lds, st, sem,
                       a.ss, K, table, n_cl, free_label, bin, a.bs, B, a.g, t.TY, labels, gt,
                       mask, h);
  });
  return launch_status();
}
