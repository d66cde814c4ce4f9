// The flash-style attention forward kernel (head dim 64), shared by the inference entry
// points (vit_block.hip) and the training forward that also records the softmax
// statistics (attention_train.hip).
#pragma once
#include <type_traits>

#include "mfma_common.h"

namespace {

// ------------------------------------------------------------------ attention
// qkv: [B, T, 3, H, 64] bf16 (the packed output of the qkv projection, q already
// scaled by head_dim^-0.5 through the weights; LOG2Q: also by log2(e), so that the
// scores arrive in the exp2 domain).  out: [B, T, H*64] bf16.
// Optional additive bias [B or 1][H or 1][T][T] fp32 (CLIP tail; strides given).
// Workgroup = 256 threads = 4 waves, 32 queries per wave.  K/V tiles of 64 keys
// go global -> LDS by DMA (global_load_lds_dwordx4, no VGPR staging) into a
// double buffer whose 16-byte chunks are XOR-swizzled by the row exactly as in
// the GEMM; one barrier per tile.  S^T = K.Q^T so the softmax statistics of a
// query are lane-local; K fragments are 16-B LDS reads, V^T fragments come from
// the hardware transposing read ds_read_b64_tr_b16.
// With head_dim 64 the loop is bound by vector issue (32 exp2 against 36 MFMAs per
// wave and tile), so the softmax is reduced to what cannot be avoided:
//  * the scores are formed RELATIVE to a per-query reference maximum: it is the C
//    operand of the first S^T MFMA (LOG2Q), so exp2 applies to the accumulator as
//    it is -- no scale, no subtraction;
//  * the reference moves only when a tile stands more than kAttRise above it
//    (guide T13); the usual tile has no rescale of O at all;
//  * the row sums come from the matrix core (a fifth V^T "d tile" of ones).
// Per wave and tile that is 32 v_exp + 16 v_cvt_pk + ~20 v_max3 + a dozen others
// (was ~200 vector instructions with the running maximum of round 2).
constexpr int HD = 64;        // head dim
constexpr int QT = 2;         // 16-query tiles per wave
constexpr int AQ = 16 * QT;   // queries per wave
constexpr int AK = 64;        // keys per LDS tile
constexpr int KV_ELEMS = AK * HD;  // one operand tile (8 KiB)
constexpr float kAttRise = 8.f;    // log2 units a score may stand above the reference maximum

typedef bf16x4 __attribute__((address_space(3))) lds_bf16x4;

// max over the four 16-lane rows of a wave without touching LDS: the gfx950
// row-swap instructions exchange halves (permlane32) / odd and even rows
// (permlane16) of two registers, so two copies of x come back as x and its
// partner.  Written as asm: through the builtin, hipcc 7.2 folds
// max(result0, result1) to result0 (seen in the ISA: both v_max dropped, rows
// disagree on their maximum).  The s_nop are the VALU-write -> swap and swap ->
// VALU-read wait states the compiler would otherwise insert itself.
__device__ __forceinline__ float max_over_rows(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  a = b = fmaxf(a, b);
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return fmaxf(a, b);
}

//
// STATS (the training forward, attention_train.hip): q is NOT pre-scaled; the scores are
// multiplied by ``c_scale`` = scale * log2(e) in the fma the natural-log form spends on
// log2(e) anyway, and the kernel also writes lse[b][h][q] = log2(l_q) - negm_q, the
// log-sum-exp of the scaled scores in log2 units (fp32, rows of ``Tp`` floats), l_q summed
// in fp32 from the weights before their half rounding (out keeps the matrix core's sum
// of the rounded ones: it is the inference kernel's to the bit).  The
// other instantiations ignore the three trailing arguments.
//
// STATS with HAS_BIAS (the CLIP tail under autograd): the bias of a (b, h) pair is a
// [Tb][Tb] matrix, Tb = T - border, rows Tb floats long.  With ``border`` = 1 it is the
// patch-to-patch matrix: token 0 has bias 0 as a query and as a key BY INDEX (bias element
// [q - 1][k - 1] for q, k >= 1), and nothing outside the matrix is read.  The inference
// instantiations ignore ``border``.  A query whose keys are all masked (bias -inf) gets an
// out row of zeros, as at inference, and lse = +inf: the backward's
// exp2(s c + bias log2(e) - lse) is then exp2(-inf) = 0, never inf - inf.  This
// instantiation holds a tile's 64 bias values next to the statistics: it is compiled for two
// workgroups per CU (at three it spilled 25 registers); the others keep three.
template <bool HAS_BIAS, bool LOG2Q, bool STATS = false>
__global__ __launch_bounds__(256, (HAS_BIAS && STATS) ? 2 : 3) void k_attention(
    const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
    int64_t bias_sb, int64_t bias_sh, int border, bf16_t* __restrict__ out, int T, int H,
    float c_scale, float* __restrict__ lse, int Tp) {
  static_assert(!STATS || !LOG2Q, "the statistics form scales the scores itself");
  __shared__ __attribute__((aligned(16))) bf16_t smem[4 * KV_ELEMS];  // [buf][K|V]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = (blockIdx.x * 4 + wave) * AQ;
  const int64_t tok_stride = (int64_t)3 * H * HD;
  const bf16_t* qb = qkv + (int64_t)b * T * tok_stride + (int64_t)h * HD;
  constexpr float kLog2e = 1.4426950408889634f;

  // DMA map (as the GEMM): wave instruction j (0..1) of wave w fills LDS rows
  // (w*2 + j)*8 .. +8 of a tile; lane l lands in row r = base + l/8, physical
  // chunk l%8, so it fetches logical chunk (l%8) ^ (r&7).  Keys beyond T are
  // clamped to the last row (masked out of the softmax below).
  int dr[2], dc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    dr[j] = (wave * 2 + j) * 8 + (lane >> 3);
    dc[j] = ((lane & 7) ^ (dr[j] & 7)) * 8;
  }
  const rsrc_t rsQ = make_rsrc(qb);   // K rows at +H*HD elements, V rows at +2*H*HD
  auto dma = [&](int buf, int k0) {
    bf16_t* dK = smem + buf * 2 * KV_ELEMS;
    bf16_t* dV = dK + KV_ELEMS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int key = k0 + dr[j] < T ? k0 + dr[j] : T - 1;
      // byte offset inside this image's qkv rows (the launcher checks < 2^31)
      const int off = 2 * (key * (int)tok_stride + dc[j]);
      const int slot = (wave * 2 + j) * 512;  // bf16 elements: 64 lanes x 8
      // buffer_load ... lds, not global_load_lds: keeps hipcc's counted lgkmcnt
      // waits on the fragment reads
      buffer_load_lds16(rsQ, (lptr_t)(dK + slot), off, 2 * H * HD);
      buffer_load_lds16(rsQ, (lptr_t)(dV + slot), off, 4 * H * HD);
    }
  };
  dma(0, 0);

  // Q fragments (B operand of S^T = K . Q^T): lane holds Q[q = fr][d = 8fg + j]
  bf16x8 qf[QT][2];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int q = q0 + i * 16 + fr;
    const int qc = q < T ? q : T - 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[i][ks] = *reinterpret_cast<const bf16x8*>(qb + (int64_t)qc * tok_stride +
                                                   ks * 32 + fg * 8);
  }
  f32x4 o[QT][4];  // [q tile][d tile]: O^T[d = 4fg + reg][q = fr]
  // ol: the row sums, accumulated by the matrix core as a fifth "d tile" whose V^T
  // fragment is all ones (every register of a lane = the sum of query fr).
  // negm: minus the REFERENCE maximum of query fr (log2 domain), in all four
  // registers: it is the C operand of the first S^T MFMA, so the scores arrive
  // already shifted.
  f32x4 ol[QT];
  float negm[QT];
  // STATS: the lane's share of the row sum of the weights BEFORE their half rounding (its
  // 16 keys of every tile, as a register pair).  lse is taken from it: the backward
  // rebuilds p = exp2(s c - lse) unrounded, and the largest weight of a row is not 1 here
  // (the reference stands up to kAttRise below the maximum), so the sum of the rounded
  // weights of a saturated row carries the full half rounding of that one weight.
  f32x2 lsum[QT];
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    ol[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    negm[i] = 0.f;
    lsum[i] = f32x2{0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = f2bf(1.f);
  const float* brow[QT];
  bool bq[QT];   // STATS: the query has a bias row (it is not the bordered class token)
  const int bd = STATS ? border : 0;
  if (HAS_BIAS) {
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      const int q = q0 + i * 16 + fr;
      const int qr = (q < T ? q : T - 1) - bd;
      bq[i] = qr >= 0;
      brow[i] = bias + b * bias_sb + h * bias_sh +
                (int64_t)(STATS && qr < 0 ? 0 : qr) * (T - bd);
    }
  }
  // fragment read offsets (bf16 elements) inside a tile
  const int offK = fr * HD + ((fg ^ (fr & 7)) * 8);  // + kt*16*HD, ^32 for ks=1
  int offV[4];  // transposing read: lane 4q+p of a 16-lane group addresses row
                // q, columns 4p..4p+3 of a 4 x 16 block (guide T10)
  {
    const int row = 4 * fg + (fr >> 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int chunk = 2 * j + ((fr & 3) >> 1);
      offV[j] = row * HD + ((chunk ^ (row & 7)) * 8) + 4 * (fr & 1);
    }
  }

  const int nt = (T + AK - 1) / AK;
  auto tile = [&](int t, auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int k0 = t * AK;
    const bf16_t* sK = smem + (t & 1) * 2 * KV_ELEMS;
    const bf16_t* sV = sK + KV_ELEMS;
    // S^T tiles: s[i][kt][reg] = S[q = i*16 + fr][key = kt*16 + 4fg + reg], in the
    // log2 domain and relative to the reference maximum
    f32x4 s[QT][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const bf16x8 kf0 =
          *reinterpret_cast<const bf16x8*>(sK + kt * 16 * HD + offK);
      const bf16x8 kf1 =
          *reinterpret_cast<const bf16x8*>(sK + kt * 16 * HD + (offK ^ 32));
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        f32x4 a = LOG2Q ? f32x4{negm[i], negm[i], negm[i], negm[i]}
                        : f32x4{0.f, 0.f, 0.f, 0.f};
        a = mfma_16x16x32(kf0, qf[i][0], a);
        a = mfma_16x16x32(kf1, qf[i][1], a);
        s[i][kt] = a;
      }
    }
    float mx[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      if (!LOG2Q) {
        // natural-log scores: scale and shift here, on register pairs and with a real
        // (-m, -m) pair (no operand crossing in the packed FMA, see the move below)
        f32x2 nn = {negm[i], negm[i]};
        asm volatile("" : "+v"(nn));
        const float c = STATS ? c_scale : kLog2e;
        const f32x2 ll = {c, c};
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          f32x2 lo = {s[i][kt][0], s[i][kt][1]}, hi = {s[i][kt][2], s[i][kt][3]};
          lo = __builtin_elementwise_fma(lo, ll, nn);
          hi = __builtin_elementwise_fma(hi, ll, nn);
          s[i][kt] = f32x4{lo[0], lo[1], hi[0], hi[1]};
        }
      }
      if (HAS_BIAS) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int key = k0 + kt * 16 + fg * 4 + r;
            if (TAIL) key = key < T ? key : T - 1;
            float bv;
            if (STATS)   // bordered: element [q - 1][key - 1], zero for token 0
              bv = (bq[i] && key >= bd) ? brow[i][key - bd] : 0.f;
            else
              bv = brow[i][key];
            s[i][kt][r] = fmaf(bv, kLog2e, s[i][kt][r]);
          }
      }
      if (TAIL) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k0 + kt * 16 + fg * 4 + r >= T) s[i][kt][r] = -INFINITY;
      }
      float m = s[i][0][0];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, s[i][kt][r]);
      mx[i] = m;
    }
    // The reference maximum of a query moves only when a score of this tile stands
    // more than kAttRise above it, or while it is not set yet: until a tile has had a
    // finite maximum for the query, its row sum is exactly 0 (after a move the maximum
    // key contributes exp2(0) = 1, and the sum never falls below that), so "l == 0"
    // is that state, per query and without a flag.  Tile 0 is not special: when it is
    // fully masked (bias -inf), the first tile with a live key sets the reference, so
    // live scores far below zero do not underflow to a row of 0.  The decision is per
    // query (the row maximum is formed over the four lane rows first, so the lanes
    // of a query agree), and when any query of the wave moves, everything that still
    // stands at the old reference -- O, the row sums, the reference and this tile's
    // scores -- moves with it, each exactly once and BEFORE any score of the tile is
    // exponentiated (guide T13's textbook order); d = 0 leaves a query as it is.
    float d[QT];
    bool any_move = false;
#pragma unroll
    for (int i = 0; i < QT; ++i) {
      const float m = max_over_rows(mx[i]);
      d[i] = (m > kAttRise || ol[i][0] == 0.f) ? m : 0.f;
      if (d[i] == -INFINITY) d[i] = 0.f;  // a fully masked row (bias of -inf)
      any_move |= d[i] != 0.f;
    }
    if (__any(any_move)) {
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        // (the first move may go DOWN by any amount: O and the sums are 0 there, keep
        // corr finite)
        const float corr = __builtin_amdgcn_exp2f(fminf(-d[i], 100.f));
        // Both factors as REAL register pairs (x, x), and the updates written on
        // pairs: left to itself hipcc packs the scalar form into v_pk_add_f32 /
        // v_pk_mul_f32 with op_sel operand crossing (one half reading the other dword
        // of the source pair), and with "op_sel:[0,1]" the low halves in lanes 48-63
        // came back unshifted now and then (a wrong P for one key of one query; 300 of
        // 300 launches of B6 T901 H12 had such a tile, none in 3000 without the
        // crossing -- DESIGN 4b).  The empty asm keeps the pairs from being folded
        // back into one register.
        f32x2 dd = {d[i], d[i]}, cc = {corr, corr};
        asm volatile("" : "+v"(dd), "+v"(cc));
        auto on_pairs = [](f32x4& x, f32x2 f, bool mul) {
          f32x2 lo = {x[0], x[1]}, hi = {x[2], x[3]};
          if (mul) { lo *= f; hi *= f; } else { lo -= f; hi -= f; }
          x = f32x4{lo[0], lo[1], hi[0], hi[1]};
        };
#pragma unroll
        for (int j = 0; j < 4; ++j) on_pairs(o[i][j], cc, true);
        on_pairs(ol[i], cc, true);
        if (STATS) lsum[i] *= cc;
        negm[i] -= d[i];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) on_pairs(s[i][kt], dd, false);
      }
    }
    // O^T += V^T . P^T : MFMA k-slot (8fg + j) <-> key
    //   j < 4 : key tile 2*kk,   keys 4fg + j
    //   j >= 4: key tile 2*kk+1, keys 4fg + (j-4)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 pf[QT];
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        typedef unsigned __attribute__((ext_vector_type(4))) u32x4;
#pragma unroll
        for (int kt = 2 * kk; kt < 2 * kk + 2; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[i][kt][r] = __builtin_amdgcn_exp2f(s[i][kt][r]);
        if (STATS) {
#pragma unroll
          for (int kt = 2 * kk; kt < 2 * kk + 2; ++kt) {
            lsum[i] += f32x2{s[i][kt][0], s[i][kt][1]};
            lsum[i] += f32x2{s[i][kt][2], s[i][kt][3]};
          }
        }
        const u32x4 pk = {pack_bf16(s[i][2 * kk][0], s[i][2 * kk][1]),
                          pack_bf16(s[i][2 * kk][2], s[i][2 * kk][3]),
                          pack_bf16(s[i][2 * kk + 1][0], s[i][2 * kk + 1][1]),
                          pack_bf16(s[i][2 * kk + 1][2], s[i][2 * kk + 1][3])};
        pf[i] = __builtin_bit_cast(bf16x8, pk);
        ol[i] = mfma_16x16x32(ones, pf[i], ol[i]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // V^T fragment of d tile j: column d = j*16 + fr of keys {4fg..4fg+3} of
        // key tiles 2kk and 2kk+1, delivered by the transposing read
        const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(sV + (2 * kk) * 16 * HD + offV[j]));
        const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(sV + (2 * kk + 1) * 16 * HD + offV[j]));
        bf16x8 vf;
        vf[0] = v0[0]; vf[1] = v0[1]; vf[2] = v0[2]; vf[3] = v0[3];
        vf[4] = v1[0]; vf[5] = v1[1]; vf[6] = v1[2]; vf[7] = v1[3];
#pragma unroll
        for (int i = 0; i < QT; ++i)
          o[i][j] = mfma_16x16x32(vf, pf[i], o[i][j]);
      }
    }
  };

  __syncthreads();  // tile 0 landed
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) dma((t + 1) & 1, (t + 1) * AK);  // flies under this tile
    if (q0 < T) {  // waves past the last query only feed the DMA and barriers
      // (no state of the loop depends on t == 0, so nothing invites the compiler to
      // peel tile 0 out of it, which would cost 80 registers of copied accumulators)
      if ((t + 1) * AK > T)
        tile(t, std::true_type{});
      else
        tile(t, std::false_type{});
    }
    __syncthreads();  // next tile landed, this one fully consumed
  }
  // normalise and store: lane owns O[q = fr][d = j*16 + 4fg .. +3]
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int q = q0 + i * 16 + fr;
    const float l = ol[i][0];
    if (STATS) {   // before the `continue`: every lane takes part in the exchange
      // the four lane rows of a query hold 16 keys of a tile each
      float lf = lsum[i][0] + lsum[i][1];
      // (16 then 32, low to high: written out, a helper changed the code)
      lf += __shfl_xor(lf, 16);
      lf += __shfl_xor(lf, 32);
      if (q < T && fg == 0) {
        float l2 = __builtin_amdgcn_logf(lf) - negm[i];
        if (HAS_BIAS && lf == 0.f) l2 = INFINITY;   // every key masked
        lse[((int64_t)b * H + h) * Tp + q] = l2;
      }
    }
    if (q >= T) continue;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    bf16_t* op = out + ((int64_t)b * T + q) * (int64_t)H * HD + (int64_t)h * HD;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint2 w2 = {pack_bf16(o[i][j][0] * inv, o[i][j][1] * inv),
                        pack_bf16(o[i][j][2] * inv, o[i][j][3] * inv)};
      *reinterpret_cast<uint2*>(op + j * 16 + fg * 4) = w2;
    }
  }
}

}  // namespace
