/*
 * tpspp_train_dec.h -- the training entry points of the NRTR decoder and its loss (ABI 10): attention with a general key
 * mask, a causal mask and separate row strides for q and k / v (the decoder's self- and cross-attention), the target
 * embedding with its position table, and the sequence cross-entropy.  Forward and backward, exact fp32.
 *
 * A header of its own next to tpspp.h and tpspp_train_attn.h (whose types, return codes and conventions apply): device
 * pointers, no allocation, no host synchronisation, work enqueued on `stream`, 0 or a negative TPSPP_E* code with a
 * message in tpspp_last_error(); every argument is checked before anything is launched.
 *
 * replaces: the autograd of textrecog/decoders/nrtr_decoder.py:81-113 (the pad & causal mask, the valid_ratio mask, the
 *           embedding with its position table), of common/modules/transformer_module.py:24-33,71-96 (the attention inside
 *           TFDecoderLayer's two MultiHeadAttention modules) and of textrecog/losses/ce_loss.py (CELoss / TFLoss) in the
 *           training graph.
 *
 * Fixed summation orders, no atomics: every entry point is bitwise reproducible from call to call and from stream to
 * stream.
 */
#ifndef TPSPP_TRAIN_DEC_H_
#define TPSPP_TRAIN_DEC_H_

#include <stddef.h>

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Attention (the kernels, tiles, arithmetic and dropout of tpspp_train_attn.h; tpspp_attn_dropout_mask materialises the
 * dropout of these entry points as well).
 *
 * Operands
 *   q (N*Tq, C) with row stride ld_q, k and v (N*Tk, C) with the common row stride ld_kv (elements, >= C), columns
 *   contiguous: q = a (N*L, C) projection with ld_q = C next to k = kv, v = kv + C of a fused (N*T, 2C) projection with
 *   ld_kv = 2C, or the three column blocks of one (N*T, 3C) buffer with ld_q = ld_kv = 3C.  out and d_out are dense.
 *   Key j is visible to query i of image b iff
 *       j < valid_len[b]          (valid_len (N) int32 or NULL; values outside [0, Tk] are clamped),
 *       key_mask[b * Tk + j] != 0 (key_mask (N, Tk) uint8 or NULL),
 *       j <= i                    (only with causal == 1; causal is 0 or 1);
 *   all that are given combine.  Key blocks of 64 that lie wholly above the diagonal of a block of 64 queries are not
 *   read, and the dk / dv kernel does not walk the query blocks that lie wholly before its key block.
 *   A query with no visible key at all -- valid_len[b] == 0, or key 0 masked under causal for the queries up to the first
 *   visible key -- is defined as tpspp_train_attn.h defines valid_len == 0: its out row is 0, its lse -inf, its dq row 0
 *   and it adds nothing to dk / dv.  A (query, key block) pair with no visible key leaves the running maximum and sum
 *   of that query untouched: no -inf - -inf, no NaN anywhere.  Rows of dk / dv of keys that no query sees are exact zeros.
 *   With valid_len alone (key_mask == NULL, causal == 0) and ld_q == ld_kv the results are bit for bit those of
 *   tpspp_attn_train_fwd / _bwd.
 *   Limits: 1 <= Tq, Tk <= 256, C == 64 * heads, heads <= 65535, 0 <= drop_p < 1.
 *
 * out (N*Tq, C), lse (N, heads, Tq).
 */
int tpspp_attn_train_fwd_ex(const float* q, long long ld_q, const float* k, const float* v, long long ld_kv, int N, int C,
                            int heads, int Tq, int Tk, const int* valid_len, const unsigned char* key_mask, int causal,
                            float drop_p, unsigned long long seed, unsigned long long offset, float* out, float* lse,
                            tpspp_stream_t stream);

/* dq (N*Tq, C) with row stride ld_dq, dk and dv (N*Tk, C) with the common row stride ld_dkv (>= C). */
int tpspp_attn_train_bwd_ex(const float* d_out, const float* q, long long ld_q, const float* k, const float* v,
                            long long ld_kv, const float* out, const float* lse, int N, int C, int heads, int Tq, int Tk,
                            const int* valid_len, const unsigned char* key_mask, int causal, float drop_p,
                            unsigned long long seed, unsigned long long offset, float* dq, long long ld_dq, float* dk,
                            float* dv, long long ld_dkv, tpspp_stream_t stream);

/*
 * Embedding: out[b, l, :] = weight[tok[b, l], :] + pos[l, :]; tok (N, L) int32, weight (num_classes, C), pos (>= L, C),
 * out (N, L, C), all dense.  A token outside [0, num_classes) indexes nothing: its row is pos[l, :] alone (callers refuse
 * such tokens on the host, where the targets originate).
 */
int tpspp_embed_pos_fwd(const int* tok, const float* weight, const float* pos, int N, int L, int C, int num_classes,
                        float* out, tpspp_stream_t stream);

/*
 * d_weight (num_classes, C), EVERY row written: row c = the sum of dx (M, C) over the tokens tok[m] == c, m ascending
 * within fixed slices of 512 tokens (partial sums into the workspace), then the slices ascending; the padding_idx row
 * (padding_idx outside [0, num_classes): none) and the rows of classes no token names are exact zeros.  Tokens outside
 * [0, num_classes) are ignored.  ws: tpspp_embed_bwd_workspace_floats(M, num_classes, C) floats.  M == 0 returns before
 * any launch (d_weight is not written).
 */
size_t tpspp_embed_bwd_workspace_floats(long long M, int num_classes, int C);
int tpspp_embed_bwd(const float* dx, const int* tok, long long M, int C, int num_classes, int padding_idx, float* d_weight,
                    float* ws, size_t ws_floats, tpspp_stream_t stream);

/*
 * Cross-entropy of logits (N, L, K), element (b, t, k) at logits[b * s_n + t * s_l + k * s_k], against targets (N, L)
 * int32 dense.  shift (0 or 1): position t is scored against target t + 1 and position L - 1 is dropped, so there are
 * Lp = L - shift scored positions per image and logits[:, L - 1] is never read (the strided view logits[:, :-1] of a dense
 * tensor and the tensor itself are the same arguments).  A position whose target equals ignore_index, or lies outside
 * [0, K), is ignored.  One wavefront per position, 1 <= K <= 1024.
 *   loss (N, Lp): lse - logit[target], 0 where ignored;  lse (N, Lp): max + log(sum of exp(logit - max));
 *   reduction 0 (none): reduced and count may be NULL;  1 (mean), 2 (sum): reduced[0] = the sum of loss over the
 *   positions ascending in a fixed two-level order (divided by count[0] for mean), count[0] = the number of scored
 *   positions as a float.  mean over zero scored positions is 0 / 0 = NaN, as PyTorch gives.
 */
#define TPSPP_CE_NONE 0
#define TPSPP_CE_MEAN 1
#define TPSPP_CE_SUM  2
int tpspp_seq_ce_fwd(const float* logits, long long s_n, long long s_l, long long s_k, const int* targets, int N, int L,
                     int K, int shift, int ignore_index, int reduction, float* loss, float* lse, float* reduced,
                     float* count, tpspp_stream_t stream);

/*
 * d_logits (N, L, K) dense = (softmax - onehot) * g, recomputed from the logits and the forward's lse.  g: (N, Lp) for
 * reduction none, one element for sum and mean (mean also divides by count[0], the forward's).  Ignored positions and,
 * with shift, the dropped position L - 1 are written as exact zeros.
 */
int tpspp_seq_ce_bwd(const float* g, const float* logits, long long s_n, long long s_l, long long s_k, const int* targets,
                     const float* lse, const float* count, int N, int L, int K, int shift, int ignore_index, int reduction,
                     float* d_logits, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_TRAIN_DEC_H_ */
