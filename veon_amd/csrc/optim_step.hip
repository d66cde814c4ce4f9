// The parameter update that ends a training iteration on MI355X: clip_grad_norm_
// (max_norm, norm_type = 2), AdamW and the weight EMA of the reference's MEGVIIEMAHook
// (mmdet3d/core/hook/ema.py:48-59) as three launches over flat fp32 arenas, where torch runs
// a handful of small kernels per parameter and three more per state_dict entry.
//
//   k_optim_sumsq    one fp32 partial per chunk of kOptimChunk gradient elements
//   k_optim_finish   one workgroup: the partials in fp64 -> scal = {norm, coef}
//   k_optim_update   one workgroup per record (a piece of one tensor, at most one chunk):
//                    clip, decay, both moments, the step and the EMA in one pass
//
// The finish is a launch of its own so that no workgroup ever waits on another inside a
// launch.  No atomics, no read-back, no allocation; every sum below has ONE order, stated
// where it is formed, so a step is bit-reproducible.  fp32, one rounding per operation
// (-ffp-contract=off; `/` and sqrtf are correctly rounded); the same code in both flavours.
//
// The clipped gradients are NOT written back: torch scales p.grad in place, but nothing
// reads a gradient between the step and the next zero_grad, and the store would add 4 bytes
// per element to a pass that moves 36.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_common.h"
#include "lane_reduce.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kOptimChunk = 4096;                      // elements; veon_optim_chunk()
constexpr int kVecPerLane = kOptimChunk / 4 / kBlock;  // float4 loads of a lane per chunk
constexpr int kMaxBlocks = 2048;                       // streaming grids stride beyond this
constexpr int kMaxGroups = VEON_OPTIM_MAX_GROUPS;

struct GroupScalars {
  float c_decay, c_1mb1, c_b2, c_1mb2, c_step, c_bc2, c_eps;
};
struct StepScalars {
  float c_d, c_1md;
  GroupScalars g[kMaxGroups];
};

// Sum of squares of chunk c = grad[c * kOptimChunk, (c + 1) * kOptimChunk), fp32, in this
// order: lane t of the workgroup reads the float4 at index j * 256 + t of the chunk for
// j = 0..3 and adds x*x, y*y, z*z, w*w of j = 0, then of j = 1, ... to ONE accumulator that
// starts at 0 (16 additions); block_sum then runs the xor butterfly (32, 16, .., 1) inside
// each wave and adds the four waves in index order, starting from 0.
__global__ __launch_bounds__(kBlock) void k_optim_sumsq(const float4* __restrict__ grad,
                                                         int64_t n_chunks,
                                                         float* __restrict__ partials) {
  __shared__ float red[1][kWaves];
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const float4* src = grad + c * (kOptimChunk / 4);
    float4 x[kVecPerLane];
#pragma unroll
    for (int j = 0; j < kVecPerLane; ++j) x[j] = src[j * kBlock + threadIdx.x];
    float acc[1] = {0.f};
#pragma unroll
    for (int j = 0; j < kVecPerLane; ++j) {
      acc[0] += x[j].x * x[j].x;
      acc[0] += x[j].y * x[j].y;
      acc[0] += x[j].z * x[j].z;
      acc[0] += x[j].w * x[j].w;
    }
    block_sum<1, kWaves>(acc, red);
    if (threadIdx.x == 0) partials[c] = acc[0];
    __syncthreads();   // red[] is written again in the next round
  }
}

// One workgroup.  fp64: thread t adds partials t, t + 256, t + 512, ... in index order to an
// accumulator that starts at 0, then block_sum as above.  norm = fp32(sqrt(sum));
// coef = max_norm / (norm + 1e-6f) clamped to at most 1 by a comparison that is false for a
// NaN, so a NaN norm gives a NaN coef (clip_grad_norm_ with error_if_nonfinite=False).
__global__ __launch_bounds__(kBlock) void k_optim_finish(const float* __restrict__ partials,
                                                          int64_t n, float max_norm,
                                                          float* __restrict__ scal) {
  __shared__ double red[1][kWaves];
  double acc[1] = {0.0};
  for (int64_t i = threadIdx.x; i < n; i += kBlock) acc[0] += (double)partials[i];
  block_sum<1, kWaves>(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc[0]);
    const float c = max_norm / (norm + 1e-6f);
    scal[0] = norm;
    scal[1] = c > 1.0f ? 1.0f : c;
  }
}

__device__ __forceinline__ void adamw_one(float grad, float coef, const GroupScalars& s,
                                          float& p, float& m, float& v) {
  const float g = grad * coef;
  p = p * s.c_decay;
  m = m + s.c_1mb1 * (g - m);
  v = v * s.c_b2 + s.c_1mb2 * (g * g);
  p = p - s.c_step * (m / (sqrtf(v) / s.c_bc2 + s.c_eps));
}

__device__ __forceinline__ float ema_one(float e, float p, float c_d, float c_1md) {
  return e * c_d + c_1md * p;
}

// Pointers read from the record table carry no address space; as global pointers their
// accesses are global_load / global_store instead of flat ones.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T>
using global_ptr = T __attribute__((address_space(1)))*;

// T = f32x4 (16-byte accesses) or float; elements [i0, i1) of the record in units of T,
// strided over the workgroup.  g / m / v are the record's arena slices (unused when !TRAIN).
template <typename T, bool TRAIN>
__device__ __forceinline__ void update_range(int i0, int i1, float* p_, float* e_,
                                             const float* g_, float* m_, float* v_,
                                             float coef, const GroupScalars& s, float c_d,
                                             float c_1md) {
  constexpr int N = sizeof(T) / sizeof(float);
  const global_ptr<T> pp = (global_ptr<T>)p_;
  const global_ptr<T> ep = (global_ptr<T>)e_;
  const global_ptr<const T> gp = (global_ptr<const T>)g_;
  const global_ptr<T> mp = (global_ptr<T>)m_;
  const global_ptr<T> vp = (global_ptr<T>)v_;
  for (int i = i0 + threadIdx.x; i < i1; i += kBlock) {
    T p = pp[i];
    T e = p, g = p, m = p, v = p;   // placeholders of the operands this record lacks
    if (e_) e = ep[i];
    if (TRAIN) {
      g = gp[i];
      m = mp[i];
      v = vp[i];
    }
    float* pf = reinterpret_cast<float*>(&p);
    float* ef = reinterpret_cast<float*>(&e);
    float* gf = reinterpret_cast<float*>(&g);
    float* mf = reinterpret_cast<float*>(&m);
    float* vf = reinterpret_cast<float*>(&v);
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (TRAIN) adamw_one(gf[k], coef, s, pf[k], mf[k], vf[k]);
      if (e_) ef[k] = ema_one(ef[k], pf[k], c_d, c_1md);
    }
    if (TRAIN) {
      pp[i] = p;
      mp[i] = m;
      vp[i] = v;
    }
    if (e_) ep[i] = e;
  }
}

template <bool TRAIN>
__device__ __forceinline__ void update_record(const veon_optim_record& rec, const float* grad,
                                              float* m_arena, float* v_arena, float coef,
                                              const GroupScalars& s, float c_d, float c_1md) {
  const int64_t off = TRAIN ? rec.offset : 0;
  const float* g = TRAIN ? grad + off : nullptr;
  float* m = TRAIN ? m_arena + off : nullptr;
  float* v = TRAIN ? v_arena + off : nullptr;
  // the arena side of a record is 16-byte aligned by construction; the tensors decide
  const bool vec = ((reinterpret_cast<uintptr_t>(rec.p) | reinterpret_cast<uintptr_t>(rec.ema)) &
                    15) == 0;
  if (vec) {
    const int n4 = rec.count >> 2;
    update_range<f32x4, TRAIN>(0, n4, rec.p, rec.ema, g, m, v, coef, s, c_d, c_1md);
    update_range<float, TRAIN>(n4 * 4, rec.count, rec.p, rec.ema, g, m, v, coef, s, c_d, c_1md);
  } else {
    update_range<float, TRAIN>(0, rec.count, rec.p, rec.ema, g, m, v, coef, s, c_d, c_1md);
  }
}

// Workgroups stride over the records.  A record with offset >= 0 is a piece of a trained
// parameter (ema may be NULL); offset < 0 is EMA-only (p is read, ema written).  coef is
// scal[1] of k_optim_finish, or 1.0f when scal is NULL (no clipping: g = grad * 1 exactly).
__global__ __launch_bounds__(kBlock) void k_optim_update(
    const veon_optim_record* __restrict__ records, int64_t n_records,
    const float* __restrict__ grad, float* __restrict__ m_arena, float* __restrict__ v_arena,
    const float* __restrict__ scal, StepScalars sc) {
  const float coef = scal ? scal[1] : 1.0f;
  for (int64_t r = blockIdx.x; r < n_records; r += gridDim.x) {
    const veon_optim_record rec = records[r];
    if (rec.offset >= 0) {
      if (!grad) continue;   // n_groups == 0: the entry point was given no arenas
      const GroupScalars s = sc.g[rec.group & (kMaxGroups - 1)];
      update_record<true>(rec, grad, m_arena, v_arena, coef, s, sc.c_d, sc.c_1md);
    } else if (rec.ema) {
      update_record<false>(rec, nullptr, nullptr, nullptr, coef, sc.g[0], sc.c_d, sc.c_1md);
    }
  }
}

inline int stream_blocks(int64_t units) {
  return (int)(units < kMaxBlocks ? units : kMaxBlocks);
}
}  // namespace

extern "C" {

int veon_optim_chunk(void) { return kOptimChunk; }

int veon_optim_sumsq(const float* grad, int64_t n, float* partials, void* stream) {
  if (!grad || !partials || n <= 0 || n % kOptimChunk || !aligned(grad, 16))
    return VEON_ERR_BAD_ARG;
  const int64_t n_chunks = n / kOptimChunk;
  hipLaunchKernelGGL(k_optim_sumsq, dim3(stream_blocks(n_chunks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const float4*>(grad),
                     n_chunks, partials);
  return launch_status();
}

int veon_optim_clip_finish(const float* partials, int64_t n_partials, double max_norm,
                           float* scal, void* stream) {
  if (!partials || !scal || n_partials <= 0 || !(max_norm > 0.0)) return VEON_ERR_BAD_ARG;
  hipLaunchKernelGGL(k_optim_finish, dim3(1), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), partials, n_partials, (float)max_norm,
                     scal);
  return launch_status();
}

int veon_optim_update(const veon_optim_record* records, int64_t n_records, const float* grad,
                      float* exp_avg, float* exp_avg_sq, const float* scal,
                      const double* host_scalars, int n_groups, void* stream) {
  if (n_records < 0 || n_groups < 0 || n_groups > kMaxGroups || !host_scalars ||
      (n_records > 0 && !records))
    return VEON_ERR_BAD_ARG;
  if (n_groups > 0 && (!grad || !exp_avg || !exp_avg_sq || !aligned(grad, 16) ||
                       !aligned(exp_avg, 16) || !aligned(exp_avg_sq, 16)))
    return VEON_ERR_BAD_ARG;
  if (n_records == 0) return VEON_OK;
  StepScalars sc = {};
  sc.c_d = (float)host_scalars[0];
  sc.c_1md = (float)host_scalars[1];
  for (int i = 0; i < n_groups; ++i) {
    const double* h = host_scalars + 2 + i * VEON_OPTIM_GROUP_SCALARS;
    sc.g[i] = GroupScalars{(float)h[0], (float)h[1], (float)h[2], (float)h[3],
                           (float)h[4], (float)h[5], (float)h[6]};
  }
  hipLaunchKernelGGL(k_optim_update, dim3(stream_blocks(n_records)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), records, n_records, grad, exp_avg,
                     exp_avg_sq, scal, sc);
  return launch_status();
}

}  // extern "C"
