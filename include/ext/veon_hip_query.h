/*
 * veon_hip_query.h -- extension of the C ABI of libveon_hip.so / libveon_hip_f16.so
 * (include/veon_hip.h): the query cross-attention of SAN's recognition head.
 *
 * Same conventions and the same declaration style as veon_hip.h (C89 prototypes, block
 * comments only; veon_amd/_lib.py reads the argument types from THIS file into a second
 * table).  The prototype lives here, not in veon_hip.h, because the launch ledger
 * (tests/test_launch_bounds_gpu.py) closes over every prototype of veon_hip.h: see
 * DESIGN 4ae.  Status codes are those of veon_hip.h; veon_abi_version() is unchanged.
 * Paths below are relative to the reference tree.
 */
#ifndef VEON_HIP_QUERY_H_
#define VEON_HIP_QUERY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======== query_attention.hip ======================================================= */

/*
 * The attention core of `cross_attn_with_self_bias`
 * (mmdet3d/models/semantic_net/attn_helper.py:34-300; logits and bias :262-273, the
 * "self" logit and its value :274-290), called per tail block from `cross_attn_layer`
 * (:303-314) by `RecWithAttnbiasHead.forward` (clip_utils/visual.py:163-216): Q query
 * tokens attend over the memory tokens key0 .. T-1 of their image (Lk = T - key0 keys;
 * the head passes key0 = 1, `xs[i][1:]`) with an additive bias and, through ONE extra
 * logit, over themselves.  head_dim is 64.
 *
 *   q_qkv   half [B][Q][3][H][64]: the packed q / k / v projection of the query tokens,
 *           q rows pre-scaled by 64^-0.5 (q_log2 != 0: also by log2(e), the exp2-domain
 *           form, as veon_vit_attention_log2);
 *   mem_kv  half: the key row (H*64 elements) of token t of image b at
 *           mem_kv + (b*T + t) * mem_token_stride, its value row H*64 elements further
 *           on.  mem_token_stride (elements, a multiple of 8, >= 2*H*64) is 2*H*64 for a
 *           [B][T][2][H][64] buffer and 3*H*64 for the K/V part of a packed qkv buffer
 *           (then mem_kv = qkv + H*64);
 *   bias    fp32 or NULL, natural-log units: element (q, j) of pair (b, h) at
 *           bias + b*bias_batch_stride + h*bias_head_stride + q*Lk + j, strides in
 *           elements, 0 = broadcast.  -inf removes key j;
 *   out     half [B][Q][H*64].
 *
 * For query q of (b, h): s_j = q.k_j + bias_j (j < Lk), s_self = q.k_q (its own k row),
 * p = softmax([s_0 .. s_{Lk-1}, s_self]), out = sum_j p_j v_j + p_self v_q.  fp32
 * accumulation; the memory weights are rounded to half before the P.V product.  The
 * running statistics are seeded from the self key (maximum s_self, sum 1, accumulator
 * v_q), which is always finite: no row is undefined, and a query whose memory keys are all
 * masked gets its own v row bit for bit.
 *
 * One launch, no workspace, no atomics, no memset, every output element written once,
 * deterministic.  VEON_ERR_BAD_ARG: a NULL or not 16-byte-aligned q_qkv / mem_kv / out,
 * B, Q, T or H < 1, key0 outside [0, T), a bad mem_token_stride, or an operand of one
 * image (Q*3*H*64 or T*mem_token_stride halves, Q*Lk bias floats) reaching 2^31 bytes.
 */
int veon_query_attention(const void *q_qkv, const void *mem_kv, int64_t mem_token_stride,
                         const float *bias, int64_t bias_batch_stride,
                         int64_t bias_head_stride, void *out, int B, int Q, int T, int key0,
                         int H, int q_log2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VEON_HIP_QUERY_H_ */
