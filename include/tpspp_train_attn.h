/*
 * tpspp_train_attn.h -- the training entry points of the NRTR encoder's attention (ABI 9): scaled-dot-product attention
 * with the valid_ratio key mask and dropout on the probabilities, forward and backward, exact fp32.
 *
 * A header of its own next to tpspp.h (whose types, return codes and conventions apply): device pointers, no
 * allocation, no host synchronisation, work enqueued on `stream`, 0 or a negative TPSPP_E* code with a message in
 * tpspp_last_error(); every argument is checked before anything is launched.
 *
 * replaces: the autograd of common/modules/transformer_module.py:24-33,71-96 (ScaledDotProductAttention and the
 *           per-head view / transpose of MultiHeadAttention) in the training graph.
 *
 * Operands
 *   q (N*Tq, C), k and v (N*Tk, C): token-major fp32, columns contiguous, ONE row stride `ld` (in elements, >= C) for
 *   the three of them, so that the three column blocks of a fused (N*T, 3C) projection are passed without copies
 *   (q = qkv, k = qkv + C, v = qkv + 2C, ld = 3C).  Head h is columns [64h, 64h + 64): C == 64 * heads.
 *   valid_len: (N) int32 or NULL; keys j >= valid_len[b] are masked (values outside [0, Tk] are clamped).  An image
 *   with valid_len[b] == 0 has no key at all: its out rows are 0, its lse -inf and its gradients 0 (PyTorch's
 *   composition gives NaN there; tps_pp_amd's modules refuse such a length on the host).
 *   Limits: 1 <= Tq, Tk <= 256, heads <= 65535, 0 <= drop_p < 1.
 *
 * Dropout
 *   Element (b, h, i, j) of the probabilities is kept iff word (i & 3) of
 *       Philox-4x32-10(counter = {h << 16 | (i >> 2) << 8 | j,  b,  offset low,  offset high},  key = seed)
 *   is >= floor(drop_p * 2^32); kept probabilities are multiplied by 1 / (1 - drop_p).  A pure function of
 *   (seed, offset, b, h, i, j): the backward regenerates it, tpspp_attn_dropout_mask materialises it.  drop_p == 0 is
 *   the no-dropout arithmetic, bit for bit.
 *
 * Arithmetic: S = (q k^T) / 8 on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, k ascending), lse = max + log(sum of
 * exp(S - max)) with a running maximum over key blocks of 64, P = exp(S - lse), out = dropout(P) v.  The backward
 * recomputes S and P from q, k and lse.  Fixed summation orders, no atomics: both directions are bitwise reproducible
 * from call to call and from stream to stream.
 */
#ifndef TPSPP_TRAIN_ATTN_H_
#define TPSPP_TRAIN_ATTN_H_

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * out (N*Tq, C) dense = dropout(softmax(mask(q k^T / 8))) v per (image, head);  lse (N, heads, Tq) = the log-sum-exp of
 * the scaled, masked logits.  Nothing else of size Tq x Tk goes to memory.
 */
int tpspp_attn_train_fwd(const float* q, const float* k, const float* v, long long ld, int N, int C, int heads, int Tq,
                         int Tk, const int* valid_len, float drop_p, unsigned long long seed,
                         unsigned long long offset, float* out, float* lse, tpspp_stream_t stream);

/*
 * dq (N*Tq, C), dk and dv (N*Tk, C) with the common row stride ld_grad (>= C; 3C for one fused (N*T, 3C) buffer) from
 * d_out (N*Tq, C) dense and the forward's operands and results (out, lse; the same mask and dropout arguments).
 * rowsum(d_out * out) is computed here.  Rows of dk / dv that belong to masked keys are written as exact zeros.
 */
int tpspp_attn_train_bwd(const float* d_out, const float* q, const float* k, const float* v, long long ld,
                         const float* out, const float* lse, int N, int C, int heads, int Tq, int Tk,
                         const int* valid_len, float drop_p, unsigned long long seed, unsigned long long offset,
                         float* dq, float* dk, float* dv, long long ld_grad, tpspp_stream_t stream);

/*
 * mask (N, heads, Tq, Tk) uint8: 1 where the two kernels above keep the probability for (seed, offset, drop_p), 0 where
 * they drop it.  For tests and debugging.
 */
int tpspp_attn_dropout_mask(int N, int heads, int Tq, int Tk, float drop_p, unsigned long long seed,
                            unsigned long long offset, unsigned char* mask, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_TRAIN_ATTN_H_ */
