// veon_query_attention (include/ext/veon_hip_query.h): the query cross-attention of SAN's
// recognition head -- Q query tokens attend over the memory tokens of their image with an
// additive fp32 bias and, through one extra logit, over themselves
// (attn_helper.py:34-300).
//
// The kernel keeps k_attention's layout (attention_kernel.h, which is included for its
// tile constants and max_over_rows and is not changed): S^T = K.Q^T on
// v_mfma_f32_16x16x32, so the statistics of a query are lane-local; K/V tiles of 64 keys
// go global -> LDS by DMA into a double buffer of XOR-swizzled 16-byte chunks, one
// barrier per tile; V^T fragments come from the transposing LDS read; the row sums from
// the matrix core (a V^T tile of ones); scores relative to a per-query reference that
// moves only when a tile stands more than kAttRise above it.
// What differs:
//  * one 16-query tile per wave (100 queries: more waves matter more than reuse of a K
//    fragment), four waves of a workgroup share the K/V tiles of their (image, head);
//  * the queries and the memory are separate operands, the memory token stride is an
//    argument and the keys start at key0;
//  * the running statistics are SEEDED from the self key: reference = s_self = q.k_q (a
//    lane-local fp32 dot product, summed over the four lane rows in a fixed order),
//    row sum 1, accumulator v_q.  The self key is always finite, so the state "reference
//    not set yet" of k_attention does not exist here, a move of the reference only ever
//    goes up, and a row whose memory keys are all masked ends as 1 * v_q / 1: its own v
//    row bit for bit.
#include "attention_kernel.h"
#include "ext/veon_hip_query.h"

namespace {

constexpr int QA_WAVES = 4;             // waves (16-query tiles) per workgroup
constexpr int QA_QUERIES = 16 * QA_WAVES;

template <bool HAS_BIAS, bool LOG2Q>
__global__ __launch_bounds__(64 * QA_WAVES) void k_query_attention(
    const bf16_t* __restrict__ q_qkv, const bf16_t* __restrict__ mem_kv, int mem_stride,
    const float* __restrict__ bias, int64_t bias_sb, int64_t bias_sh,
    bf16_t* __restrict__ out, int Q, int T, int key0, int H) {
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * KV_ELEMS];  // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = (blockIdx.x * QA_WAVES + wave) * 16;
  const int Lk = T - key0;
  const int64_t q_stride = (int64_t)3 * H * HD;
  const bf16_t* qb = q_qkv + (int64_t)b * Q * q_stride + (int64_t)h * HD;
  // key row of memory key 0 (token key0) of this image and head; value rows H*HD further
  const bf16_t* mb = mem_kv + ((int64_t)b * T + key0) * mem_stride + (int64_t)h * HD;
  constexpr float kLog2e = 1.4426950408889634f;

  // DMA map of k_attention: wave instruction j (0..1) of wave w fills LDS rows
  // (w*2 + j)*8 .. +8 of a tile; lane l lands in row r = base + l/8, physical chunk l%8,
  // so it fetches logical chunk (l%8) ^ (r&7).  Keys beyond Lk are clamped to the last
  // key (masked out of the softmax below): nothing outside the operand is read.
  int dr[2], dc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    dr[j] = (wave * 2 + j) * 8 + (lane >> 3);
    dc[j] = ((lane & 7) ^ (dr[j] & 7)) * 8;
  }
  const rsrc_t rsM = make_rsrc(mb);
  auto dma = [&](int buf, int k0) {
    bf16_t* dK = smem + buf * 2 * KV_ELEMS;
    bf16_t* dV = dK + KV_ELEMS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int key = k0 + dr[j] < Lk ? k0 + dr[j] : Lk - 1;
      // byte offset inside this image's memory rows (the launcher checks < 2^31)
      const int off = 2 * (key * mem_stride + dc[j]);
      const int slot = (wave * 2 + j) * 512;  // half elements: 64 lanes x 8
      buffer_load_lds16(rsM, (lptr_t)(dK + slot), off, 0);
      buffer_load_lds16(rsM, (lptr_t)(dV + slot), off, 2 * H * HD);
    }
  };
  dma(0, 0);

  // the query's own rows: lane holds q / k_q [q = fr][d = ks*32 + 8fg + j] (the B operand
  // of S^T = K . Q^T) and v_q [q = fr][d = j*16 + 4fg + r] (the accumulator's layout)
  const int qi = q0 + fr < Q ? q0 + fr : Q - 1;
  const bf16_t* qrow = qb + (int64_t)qi * q_stride;
  bf16x8 qf[2];
  float self = 0.f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + ks * 32 + fg * 8);
    const bf16x8 kq = *reinterpret_cast<const bf16x8*>(qrow + H * HD + ks * 32 + fg * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      self = fmaf(bf2f((bf16_t)qf[ks][e]), bf2f((bf16_t)kq[e]), self);
  }
  // over the four lane rows of the query, 16 then 32: (a + b) + (c + d) in every lane
  // (addition commutes), so the four lanes of a query hold the same bits
  self += __shfl_xor(self, 16);
  self += __shfl_xor(self, 32);
  // negm: minus the reference maximum of query fr in log2 units, seeded with the self
  // logit; ol: the row sum (all four registers), seeded with the self weight exp2(0) = 1;
  // o: O^T[d = j*16 + 4fg + reg][q = fr], seeded with v_q
  float negm = -(LOG2Q ? self : self * kLog2e);
  f32x4 ol = f32x4{1.f, 1.f, 1.f, 1.f};
  f32x4 o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x4 vq =
        *reinterpret_cast<const bf16x4*>(qrow + 2 * H * HD + j * 16 + fg * 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[j][r] = bf2f((bf16_t)vq[r]);
  }
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = f2bf(1.f);
  // (The bias is loaded where it is used.  Fetching a tile's 16 floats per lane one tile
  // ahead, under the tile before it, was tried and was slower: 32.1 against 20.3 us at
  // B 6, H 12, Q 100, Lk 704 -- DESIGN 4ae.)
  const float* brow = nullptr;
  if (HAS_BIAS) brow = bias + b * bias_sb + h * bias_sh + (int64_t)qi * Lk;

  // fragment read offsets (half elements) inside a tile, as k_attention
  const int offK = fr * HD + ((fg ^ (fr & 7)) * 8);  // + kt*16*HD, ^32 for ks=1
  int offV[4];
  {
    const int row = 4 * fg + (fr >> 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int chunk = 2 * j + ((fr & 3) >> 1);
      offV[j] = row * HD + ((chunk ^ (row & 7)) * 8) + 4 * (fr & 1);
    }
  }

  const int nt = (Lk + AK - 1) / AK;
  auto tile = [&](int t, auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int k0 = t * AK;
    const bf16_t* sK = smem + (t & 1) * 2 * KV_ELEMS;
    const bf16_t* sV = sK + KV_ELEMS;
    // s[kt][reg] = S[q = fr][key = k0 + kt*16 + 4fg + reg], log2 units, relative to the
    // reference
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 kf0 = *reinterpret_cast<const bf16x8*>(sK + kt * 16 * HD + offK);
      const bf16x8 kf1 = *reinterpret_cast<const bf16x8*>(sK + kt * 16 * HD + (offK ^ 32));
      f32x4 a = LOG2Q ? f32x4{negm, negm, negm, negm} : f32x4{0.f, 0.f, 0.f, 0.f};
      a = mfma_16x16x32(kf0, qf[0], a);
      a = mfma_16x16x32(kf1, qf[1], a);
      s[kt] = a;
    }
    if (!LOG2Q) {
      // natural-log scores: scale and shift here, on register pairs with a real (-m, -m)
      // pair (no operand crossing in the packed FMA: DESIGN 4b)
      f32x2 nn = {negm, negm};
      asm volatile("" : "+v"(nn));
      const f32x2 ll = {kLog2e, kLog2e};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x2 lo = {s[kt][0], s[kt][1]}, hi = {s[kt][2], s[kt][3]};
        lo = __builtin_elementwise_fma(lo, ll, nn);
        hi = __builtin_elementwise_fma(hi, ll, nn);
        s[kt] = f32x4{lo[0], lo[1], hi[0], hi[1]};
      }
    }
    if (HAS_BIAS) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int key = k0 + kt * 16 + fg * 4 + r;
          if (TAIL) key = key < Lk ? key : Lk - 1;
          s[kt][r] = fmaf(brow[key], kLog2e, s[kt][r]);
        }
    }
    if (TAIL) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + kt * 16 + fg * 4 + r >= Lk) s[kt][r] = -INFINITY;
    }
    float mx = s[0][0];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    // The reference of a query moves only when a score of this tile stands more than
    // kAttRise above it (the decision is per query: the maximum is formed over the four
    // lane rows first).  It was seeded with the self logit, so it is always set and only
    // ever rises; a fully masked tile (maximum -inf) never moves it.  When any query of
    // the wave moves, O, the row sum, the reference and this tile's scores move with it,
    // each once and BEFORE any score of the tile is exponentiated.
    const float m = max_over_rows(mx);
    const float d = m > kAttRise ? m : 0.f;
    if (__any(d != 0.f)) {
      const float corr = __builtin_amdgcn_exp2f(-d);
      // both factors as REAL register pairs and the updates written on pairs: the scalar
      // form is packed by hipcc into v_pk_* with op_sel operand crossing
      f32x2 dd = {d, d}, cc = {corr, corr};
      asm volatile("" : "+v"(dd), "+v"(cc));
      auto on_pairs = [](f32x4& x, f32x2 f, bool mul) {
        f32x2 lo = {x[0], x[1]}, hi = {x[2], x[3]};
        if (mul) { lo *= f; hi *= f; } else { lo -= f; hi -= f; }
        x = f32x4{lo[0], lo[1], hi[0], hi[1]};
      };
#pragma unroll
      for (int j = 0; j < 4; ++j) on_pairs(o[j], cc, true);
      on_pairs(ol, cc, true);
      negm -= d;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) on_pairs(s[kt], dd, false);
    }
    // O^T += V^T . P^T : MFMA k-slot (8fg + j) <-> key
    //   j < 4 : key tile 2*kk,   keys 4fg + j
    //   j >= 4: key tile 2*kk+1, keys 4fg + (j-4)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      typedef unsigned __attribute__((ext_vector_type(4))) u32x4;
#pragma unroll
      for (int kt = 2 * kk; kt < 2 * kk + 2; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r]);
      const u32x4 pk = {pack_bf16(s[2 * kk][0], s[2 * kk][1]),
                        pack_bf16(s[2 * kk][2], s[2 * kk][3]),
                        pack_bf16(s[2 * kk + 1][0], s[2 * kk + 1][1]),
                        pack_bf16(s[2 * kk + 1][2], s[2 * kk + 1][3])};
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pk);
      ol = mfma_16x16x32(ones, pf, ol);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(sV + (2 * kk) * 16 * HD + offV[j]));
        const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(sV + (2 * kk + 1) * 16 * HD + offV[j]));
        bf16x8 vf;
        vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
        vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
        o[j] = mfma_16x16x32(vf, pf, o[j]);
      }
    }
  };

  __syncthreads();  // tile 0 landed
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) dma((t + 1) & 1, (t + 1) * AK);  // flies under this tile
    if (q0 < Q) {  // waves past the last query only feed the DMA and the barriers
      if ((t + 1) * AK > Lk)
        tile(t, std::true_type{});
      else
        tile(t, std::false_type{});
    }
    __syncthreads();  // next tile landed, this one fully consumed
  }
  // normalise and store: lane owns O[q = fr][d = j*16 + 4fg .. +3]; the row sum is at
  // least the last reference holder's weight, never 0
  const int q = q0 + fr;
  if (q >= Q) return;
  const float l = ol[0];
  const float inv = l > 0.f ? 1.f / l : 0.f;
  bf16_t* op = out + ((int64_t)b * Q + q) * (int64_t)H * HD + (int64_t)h * HD;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint2 w2 = {pack_bf16(o[j][0] * inv, o[j][1] * inv),
                      pack_bf16(o[j][2] * inv, o[j][3] * inv)};
    *reinterpret_cast<uint2*>(op + j * 16 + fg * 4) = w2;
  }
}

}  // namespace

int veon_query_attention(const void* q_qkv, const void* mem_kv, int64_t mem_token_stride,
                         const float* bias, int64_t bias_batch_stride,
                         int64_t bias_head_stride, void* out, int B, int Q, int T, int key0,
                         int H, int q_log2, void* stream) {
  if (!q_qkv || !mem_kv || !out || B < 1 || Q < 1 || T < 1 || H < 1) return VEON_ERR_BAD_ARG;
  if (key0 < 0 || key0 >= T) return VEON_ERR_BAD_ARG;
  if (B > 65535 || H > 65535) return VEON_ERR_BAD_ARG;   // grid y / z
  if (!al16(q_qkv) || !al16(mem_kv) || !al16(out)) return VEON_ERR_BAD_ARG;
  if (bias && !aligned(bias, 4)) return VEON_ERR_BAD_ARG;
  if (bias && (bias_batch_stride < 0 || bias_head_stride < 0)) return VEON_ERR_BAD_ARG;
  // a key and its value row lie inside one token's stride; 16-byte DMA chunks
  if (mem_token_stride < (int64_t)2 * H * HD || mem_token_stride % 8 != 0)
    return VEON_ERR_BAD_ARG;
  // the kernel addresses an image's rows with 32-bit byte offsets
  const int64_t lim = 1ll << 31;
  if (mem_token_stride >= lim || (int64_t)T * mem_token_stride * 2 >= lim ||
      (int64_t)Q * 3 * H * HD * 2 >= lim || (int64_t)Q * (T - key0) * 4 >= lim)
    return VEON_ERR_BAD_ARG;
  const dim3 grid((unsigned)((Q + QA_QUERIES - 1) / QA_QUERIES), (unsigned)H, (unsigned)B);
#define VEON_LAUNCH_QA(BIAS, LOG2Q)                                                   \
  hipLaunchKernelGGL((k_query_attention<BIAS, LOG2Q>), grid, dim3(64 * QA_WAVES), 0,  \
                     static_cast<hipStream_t>(stream),                                \
                     static_cast<const bf16_t*>(q_qkv),                               \
                     static_cast<const bf16_t*>(mem_kv), (int)mem_token_stride, bias, \
                     bias_batch_stride, bias_head_stride, static_cast<bf16_t*>(out),  \
                     Q, T, key0, H)
  if (q_log2) {
    if (bias != nullptr) VEON_LAUNCH_QA(true, true); else VEON_LAUNCH_QA(false, true);
  } else {
    if (bias != nullptr) VEON_LAUNCH_QA(true, false); else VEON_LAUNCH_QA(false, false);
  }
#undef VEON_LAUNCH_QA
  return launch_status();
}
