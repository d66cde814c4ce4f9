// On-device Occ3D F-score (Metric_FScore, mmdet3d/datasets/occ_metrics.py:150-237): the
// four integer counts per sample from which accuracy, completeness and their harmonic
// mean follow -- without the reference's two KD-trees.
//
// Both point sets of the reference are voxel centres of ONE lattice, so "the nearest
// point of the other set is closer than the threshold" is "the other set holds a voxel at
// an integer offset inside the threshold's ball".  The ball is a table of reaches: for
// every (dx, dy) the largest |dz| inside it, or -1 (veon_amd/occ_eval.py: fscore_reach,
// which also refuses thresholds that a lattice distance comes too close to).
//
// Bit-packed columns.  With Z <= 64 one (x, y) column is ONE 64-bit word, bit z set where
// the voxel is occupied (its label is not void and its mask is not 0).  The neighbourhood
// test of a whole column is then: OR over the table's (dx, dy) of the neighbour column's
// word spread by +-reach in z (shifts), AND with the own word, population count.
//
// Mapping.  A block owns tiles of T x T columns of one sample and strides over the tiles
// of the bounded grid.  Phase 1: its threads (lanes along y, the direction in which
// columns follow each other in memory) read the Z bytes of every column of the tile and of
// a halo of H = max(R_acc, R_cmpl) columns around it -- 16, 8 or 4 bytes per load when Z
// and the pointers allow, else bytes; int64 predictions element by element -- and leave
// the two words of each column (prediction, ground truth) in LDS.  A column outside the
// sample's (X, Y) grid is two zero words: never a column of the neighbouring sample, never
// the wrap-around of a flat index.  Phase 2, after a barrier: one thread per column of the
// tile forms the two neighbourhood words and counts.  Bits at or above Z are never set in
// a word, and a spread that pushes bits there is ANDed with such a word, so no Z-bit mask
// is formed at all (and nothing is shifted by 64 at Z = 64).
//
// Reduction.  n_pred, n_gt, hit_pred, hit_gt of the tile: wave shuffles, then LDS across
// the four waves, then at most four 64-bit integer atomics into row b of counts.  Integer
// sums: exact and independent of the order.  Nothing is allocated or read back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int T = 16;             // a tile is T x T columns: one per thread in phase 2
constexpr int MAX_R = 3;          // largest halo
constexpr int MAX_SIDE = 2 * MAX_R + 1;
constexpr int MAX_TAB = MAX_SIDE * MAX_SIDE;
constexpr int MAX_HW = T + 2 * MAX_R;
constexpr int MAX_BLOCKS = 2048;  // grid bound; more tiles are strided over
constexpr int MAX_Z = 64;

template <int W> struct Bytes;
template <> struct Bytes<1> { using V = uint8_t; };
template <> struct Bytes<4> { using V = uint32_t; };
template <> struct Bytes<8> { using V = uint2; };
template <> struct Bytes<16> { using V = uint4; };

// by value in the kernel's arguments: nothing lives in device memory between calls
struct Tables {
  unsigned long long void_words[4];   // bit v of word v / 64: label v is void
  int r_acc, r_cmpl;
  signed char acc[MAX_TAB];           // (2 r_acc + 1)^2 reaches, [dx + r][dy + r]
  signed char cmpl[MAX_TAB];
};

// the word with every bit within +-r of a set bit of w
__device__ __forceinline__ unsigned long long spread(unsigned long long w, int r) {
  for (int k = 0; k < r; ++k) w |= (w << 1) | (w >> 1);
  return w;
}

// The two occupancy words of the column that starts at element `off`.
template <typename P, int W>
__device__ __forceinline__ ulonglong2 column(const P* __restrict__ pred,
                                             const uint8_t* __restrict__ gt,
                                             const uint8_t* __restrict__ mask, int64_t off,
                                             int Z, const uint8_t* is_void) {
  using V = typename Bytes<W>::V;
  unsigned long long pw = 0ull, gw = 0ull;
  for (int k = 0; k < Z; k += W) {   // Z % W == 0
    const V gv = *reinterpret_cast<const V*>(gt + off + k);
    V mv = gv, pv = gv;              // any value: unread without a mask / for int64 labels
    if (mask) mv = *reinterpret_cast<const V*>(mask + off + k);
    if (sizeof(P) == 1) pv = *reinterpret_cast<const V*>(pred + off + k);
    const uint8_t* gb = reinterpret_cast<const uint8_t*>(&gv);
    const uint8_t* mb = reinterpret_cast<const uint8_t*>(&mv);
    const uint8_t* pb = reinterpret_cast<const uint8_t*>(&pv);
    unsigned pbits = 0u, gbits = 0u;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      bool p_occ;
      if (sizeof(P) == 1) {
        p_occ = !is_void[pb[j]];
      } else {   // outside [0, 255]: equal to no void label, so occupied
        const int64_t v = (int64_t)pred[off + k + j];
        p_occ = (uint64_t)v > 255ull || !is_void[(int)v];
      }
      const bool seen = !mask || mb[j];
      pbits |= (unsigned)(seen && p_occ) << j;
      gbits |= (unsigned)(seen && !is_void[gb[j]]) << j;
    }
    pw |= (unsigned long long)pbits << k;   // k <= 63
    gw |= (unsigned long long)gbits << k;
  }
  return make_ulonglong2(pw, gw);
}

template <typename P, int W>
__global__ __launch_bounds__(THREADS) void k_occ_fscore(
    const P* __restrict__ pred, const uint8_t* __restrict__ gt,
    const uint8_t* __restrict__ mask, int B, int X, int Y, int Z, Tables tab,
    unsigned long long* __restrict__ counts) {
  __shared__ ulonglong2 words[MAX_HW * MAX_HW];   // .x prediction, .y ground truth
  __shared__ uint8_t is_void[256];
  __shared__ signed char reach[2][MAX_TAB];
  __shared__ unsigned red[WAVES][4];
  const int tid = threadIdx.x;
  {
    const unsigned long long w = tab.void_words[tid >> 6];
    is_void[tid] = (uint8_t)((w >> (tid & 63)) & 1ull);
    if (tid < MAX_TAB) {
      reach[0][tid] = tab.acc[tid];
      reach[1][tid] = tab.cmpl[tid];
    }
  }
  __syncthreads();
  const int ra = tab.r_acc, rc = tab.r_cmpl;
  const int H = ra > rc ? ra : rc, HW = T + 2 * H;
  const int tiles_x = (X + T - 1) / T, tiles_y = (Y + T - 1) / T;
  const int tiles = B * tiles_x * tiles_y;   // <= B*X*Y < 2^31
  const int xl = tid / T, yl = tid % T;      // the own column in phase 2
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int ty = t % tiles_y, tx = (t / tiles_y) % tiles_x, b = t / (tiles_x * tiles_y);
    const int x0 = tx * T - H, y0 = ty * T - H;
    for (int i = tid; i < HW * HW; i += THREADS) {
      const int x = x0 + i / HW, y = y0 + i % HW;
      ulonglong2 w = make_ulonglong2(0ull, 0ull);
      if (x >= 0 && x < X && y >= 0 && y < Y)
        w = column<P, W>(pred, gt, mask, (((int64_t)b * X + x) * Y + y) * Z, Z, is_void);
      words[i] = w;
    }
    __syncthreads();

    const ulonglong2 own = words[(xl + H) * HW + yl + H];   // zeros outside the grid
    unsigned c[4] = {(unsigned)__popcll(own.x), (unsigned)__popcll(own.y), 0u, 0u};
    if (own.x) {   // ground truth within reach_acc of the predicted voxels
      unsigned long long near = 0ull;
      const int side = 2 * ra + 1;
      for (int dx = -ra; dx <= ra; ++dx)
        for (int dy = -ra; dy <= ra; ++dy) {
          const int r = reach[0][(dx + ra) * side + dy + ra];
          if (r >= 0) near |= spread(words[(xl + H + dx) * HW + yl + H + dy].y, r);
        }
      c[2] = (unsigned)__popcll(own.x & near);
    }
    if (own.y) {   // predictions within reach_cmpl of the ground-truth voxels
      unsigned long long near = 0ull;
      const int side = 2 * rc + 1;
      for (int dx = -rc; dx <= rc; ++dx)
        for (int dy = -rc; dy <= rc; ++dy) {
          const int r = reach[1][(dx + rc) * side + dy + rc];
          if (r >= 0) near |= spread(words[(xl + H + dx) * HW + yl + H + dy].x, r);
        }
      c[3] = (unsigned)__popcll(own.y & near);
    }
    // (integer counts by __shfl_down into lane 0 and red[wave][k]: not block_sum's layout)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) c[k] += __shfl_down(c[k], s, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[tid >> 6][k] = c[k];
    }
    __syncthreads();   // the words are free again; the waves' sums are in place
    if (tid < 4) {     // (read before this thread passes the next tile's barrier)
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) sum += red[w][tid];
      if (sum) atomicAdd(counts + (int64_t)b * 4 + tid, (unsigned long long)sum);
    }
  }
}

// (2r + 1)^2 reaches in [-1, 63] from a host array into the kernel's table
bool take_reaches(int r, const int* src, signed char* dst) {
  if (r < 0 || r > MAX_R || !src) return false;
  const int n = (2 * r + 1) * (2 * r + 1);
  for (int i = 0; i < MAX_TAB; ++i) dst[i] = -1;
  for (int i = 0; i < n; ++i) {
    if (src[i] < -1 || src[i] >= MAX_Z) return false;
    dst[i] = (signed char)src[i];
  }
  return true;
}

template <typename P>
void launch(int W, int blocks, hipStream_t st, const void* pred, const uint8_t* gt,
            const uint8_t* mask, int B, int X, int Y, int Z, const Tables& tab,
            unsigned long long* counts) {
#define VEON_FSCORE(w)                                                                   \
  hipLaunchKernelGGL((k_occ_fscore<P, w>), dim3((unsigned)blocks), dim3(THREADS), 0, st, \
                     static_cast<const P*>(pred), gt, mask, B, X, Y, Z, tab, counts)
  switch (W) {
    case 16: VEON_FSCORE(16); break;
    case 8: VEON_FSCORE(8); break;
    case 4: VEON_FSCORE(4); break;
    default: VEON_FSCORE(1); break;
  }
#undef VEON_FSCORE
}

}  // namespace

extern "C" int veon_occ_fscore_counts(const void* pred, int pred_elem_bytes,
                                      const uint8_t* gt, const uint8_t* mask, int B, int X,
                                      int Y, int Z, const int64_t* void_words, int r_acc,
                                      const int* reach_acc, int r_cmpl,
                                      const int* reach_cmpl, int64_t* counts, void* stream) {
  if (!pred || !gt || !counts || !void_words ||
      (pred_elem_bytes != 1 && pred_elem_bytes != 8) || !aligned(pred, pred_elem_bytes) ||
      !aligned(counts, 8) || B <= 0 || X <= 0 || Y <= 0 || Z <= 0 || Z > MAX_Z)
    return VEON_ERR_BAD_ARG;
  if ((int64_t)B * X * Y * Z > 0x7fffffffLL) return VEON_ERR_BAD_ARG;
  Tables tab;
  for (int i = 0; i < 4; ++i) tab.void_words[i] = (unsigned long long)void_words[i];
  tab.r_acc = r_acc;
  tab.r_cmpl = r_cmpl;
  if (!take_reaches(r_acc, reach_acc, tab.acc) || !take_reaches(r_cmpl, reach_cmpl, tab.cmpl))
    return VEON_ERR_BAD_ARG;
  int W = 1;
  for (int w : {16, 8, 4}) {
    if (Z % w == 0 && aligned(gt, w) && aligned(mask, w) &&
        (pred_elem_bytes == 8 || aligned(pred, w))) {
      W = w;
      break;
    }
  }
  const int64_t tiles = (int64_t)B * ((X + T - 1) / T) * ((Y + T - 1) / T);
  const int blocks = even_share_blocks(tiles, MAX_BLOCKS);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  if (pred_elem_bytes == 1)
    launch<uint8_t>(W, blocks, st, pred, gt, mask, B, X, Y, Z, tab, c);
  else
    launch<int64_t>(W, blocks, st, pred, gt, mask, B, X, Y, Z, tab, c);
  return launch_status();
}
