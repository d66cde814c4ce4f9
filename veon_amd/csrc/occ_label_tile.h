// The tile walk of the label-only tails (occ_tail.hip: k_occ_labels, k_occ_labels_grouped):
// one definition of the mapping, the LDS staging of whole z columns,
// the W-byte output and the LDS integer counters of the fused confusion matrix.  The two
// kernels differ only in the label of a voxel, which they pass in as a functor.
//
// Mapping.  A block owns tiles of TX x TY (x,y) columns, every z of them.  Lanes walk
// x fastest, then y, then z -- the order of the low-resolution rows, as in
// k_occ_classify -- and drop each label as one byte into LDS at its place in the
// (x, y, z) order of the output.  After a barrier the tile is written out as runs of
// TY*Zo contiguous bytes per x, W = 16 / 8 / 4 / 1 bytes per lane (the largest that
// divides Zo and the alignment of the pointers); the ground truth and the mask are
// read with the same W-byte accesses at the same offsets.
//
// Histogram.  n_cl*n_cl 32-bit counters in LDS, zeroed once per block; every voxel
// with mask != 0 and gt < n_cl adds 1 to counter n_cl*gt + label with an LDS integer
// atomic (a lane first merges equal neighbours among its W voxels: one z column is
// mostly one class).  The grid is bounded and strides over the tiles, and after the
// last tile each block adds its non-zero counters to the global int64 histogram with
// 64-bit integer atomics.  Integer sums: exact and independent of the order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"
#include "occ_interp.h"

namespace {

constexpr int THREADS = 256;
constexpr int TX = 16;            // x columns of a tile
constexpr int TILE_VOXELS = 1024; // TY is chosen for about this many voxels per tile
constexpr int MAX_BLOCKS = 2048;  // grid bound; more work is strided over
constexpr int MAX_CL = 64;        // 64*64 counters = 16 KB of LDS
constexpr int MAX_ZO = 2048;      // TX*Zo bytes of staged labels = 32 KB of LDS

template <int W> struct Bytes;
template <> struct Bytes<1> { using T = uint8_t; };
template <> struct Bytes<4> { using T = uint32_t; };
template <> struct Bytes<8> { using T = uint2; };
template <> struct Bytes<16> { using T = uint4; };

__device__ __forceinline__ void zero_counters(unsigned* cnt, int n_cl) {
  for (int i = threadIdx.x; i < n_cl * n_cl; i += THREADS) cnt[i] = 0u;
}

// after a barrier: the block's non-zero counters into the global histogram
__device__ __forceinline__ void flush_counters(const unsigned* cnt, int n_cl,
                                               unsigned long long* __restrict__ hist) {
  for (int i = threadIdx.x; i < n_cl * n_cl; i += THREADS) {
    const unsigned c = cnt[i];
    if (c) atomicAdd(hist + i, (unsigned long long)c);
  }
}

// The whole kernel body: `label(b, z, y, x)` -> the voxel's label, below n_cl wherever a
// histogram is given.  `smem`: 16-byte aligned LDS of tile_lds_bytes().
template <int W, typename Label>
__device__ __forceinline__ void label_tiles(
    unsigned char* smem, Label label, int n_cl, int B, const Grid& g, int TY,
    uint8_t* __restrict__ labels, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, unsigned long long* __restrict__ hist) {
  using T = typename Bytes<W>::T;
  const int Zo = g.Zo, Yo = g.Yo, Xo = g.Xo;
  const int col = TY * Zo;   // staged bytes of one x of the tile, (y, z) order
  uint8_t* stage = smem;
  unsigned* cnt = reinterpret_cast<unsigned*>(smem + ((TX * col + 15) & ~15));
  if (hist) zero_counters(cnt, n_cl);   // (the first barrier below orders it)

  const int tiles_x = (Xo + TX - 1) / TX, tiles_y = (Yo + TY - 1) / TY;
  const int tiles = B * tiles_y * tiles_x;   // <= B*Yo*Xo < 2^31
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
    const int x0 = tx * TX, y0 = ty * TY;
    const int nx = Xo - x0 < TX ? Xo - x0 : TX, ny = Yo - y0 < TY ? Yo - y0 : TY;

    for (int i = threadIdx.x; i < TX * col; i += THREADS) {
      const int xl = i % TX, r = i / TX;
      const int yl = r % TY, z = r / TY;
      if (xl < nx && yl < ny)
        stage[xl * col + yl * Zo + z] = (uint8_t)label(b, z, y0 + yl, x0 + xl);
    }
    __syncthreads();

    // ny*Zo contiguous bytes per x, in LDS and in the output; Zo % W == 0
    const int units = ny * Zo / W;
    for (int u = threadIdx.x; u < nx * units; u += THREADS) {
      const int xl = u / units, k = u - xl * units;
      const int64_t off = (((int64_t)b * Xo + x0 + xl) * Yo + y0) * Zo + (int64_t)k * W;
      const T lab = *reinterpret_cast<const T*>(stage + xl * col + k * W);
      *reinterpret_cast<T*>(labels + off) = lab;
      if (hist) {
        const T gv = *reinterpret_cast<const T*>(gt + off);
        T mv = gv;   // any value: unread without a mask
        if (mask) mv = *reinterpret_cast<const T*>(mask + off);
        const uint8_t* lb = reinterpret_cast<const uint8_t*>(&lab);
        const uint8_t* gb = reinterpret_cast<const uint8_t*>(&gv);
        const uint8_t* mb = reinterpret_cast<const uint8_t*>(&mv);
        int run_bin = 0;
        unsigned run = 0u;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          if ((!mask || mb[j]) && gb[j] < n_cl) {
            const int bin_j = gb[j] * n_cl + lb[j];   // label < n_cl
            if (run && bin_j != run_bin) {
              atomicAdd(cnt + run_bin, run);
              run = 0u;
            }
            run_bin = bin_j;
            ++run;
          }
        }
        if (run) atomicAdd(cnt + run_bin, run);
      }
    }
    __syncthreads();   // the stage is free again; after the last tile: counters complete
  }
  if (hist) flush_counters(cnt, n_cl, hist);
}

// The launch shape of label_tiles for one problem.
struct TileLaunch {
  int TY, W, blocks;
  size_t lds;   // of label_tiles alone
};

inline TileLaunch tile_launch(int B, int Zo, int Yo, int Xo, int n_cl, const uint8_t* labels,
                              const uint8_t* gt, const uint8_t* mask, bool hist) {
  // about four voxels per thread and tile (16 x 4 columns of 16 at the VEON shape, 650
  // tiles): measured against one, two and eight, it is the fastest with and without the
  // histogram -- fewer barriers and fewer blocks that flush counters, still every SIMD busy
  TileLaunch t;
  t.TY = TILE_VOXELS / (TX * Zo);
  t.TY = t.TY < 1 ? 1 : (t.TY > Yo ? Yo : t.TY);
  t.W = 1;
  for (int w : {16, 8, 4}) {
    if (Zo % w == 0 && aligned(labels, w) && aligned(gt, w) && aligned(mask, w)) {
      t.W = w;
      break;
    }
  }
  const int64_t tiles = (int64_t)B * ((Yo + t.TY - 1) / t.TY) * ((Xo + TX - 1) / TX);
  t.blocks = even_share_blocks(tiles, MAX_BLOCKS);
  t.lds = (size_t)((TX * t.TY * Zo + 15) & ~15) + (hist ? sizeof(unsigned) * n_cl * n_cl : 0);
  return t;
}

}  // namespace
