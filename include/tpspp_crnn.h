/*
 * tpspp_crnn.h -- the CRNN recogniser behind the classic TPS rectifier (configs/_base_/recog_models/crnn_tps.py):
 * what VeryDeepVgg, CRNNDecoder(rnn_flag=True) and CTCConvertor need beyond the entry points of tpspp.h.
 *
 * tpspp.h's types, return codes and conventions apply: device pointers, no allocation, no host synchronisation, work
 * enqueued on `stream`, 0 or a negative TPSPP_E* code with a message in tpspp_last_error(); every argument is checked
 * before anything is launched.  TPSPP_ABI_VERSION is not raised by it: a library that lacks one of these symbols fails to
 * bind by name.
 *
 * replaces: nn.MaxPool2d(2, 2) and nn.MaxPool2d((2, 2), (2, 1), (0, 1))     backbones/very_deep_vgg.py:51-60
 *           the recurrence of nn.LSTM(nIn, 256, bidirectional=True)        layers/lstm_layer.py:10,14
 *           F.softmax, topk(1) and the collapse scan of tensor2idx         convertors/ctc.py:110-137
 * The rest of the model runs on tpspp.h: the 3x3 convolutions, and conv6 (2x2, valid) as a 3x3 kernel with a zero first
 * row and column at stride (2, 1), on tpspp_conv2d_fwd; the LSTM input projections, the embedding Linears and the
 * (W, N, C) -> (N, W, C) permutation on tpspp_mm_f32.
 *
 * "float" is IEEE fp32; nothing is contracted beyond the fused multiply-adds written below.
 */
#ifndef TPSPP_CRNN_H_
#define TPSPP_CRNN_H_

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TPSPP_CRNN_HIDDEN 256   /* the reference hard-codes it: crnn_decoder.py:35-36 */

/*
 * nn.MaxPool2d((kh, kw), (sh, sw), (ph, pw)), ceil_mode = False, dilation 1: in (N, C, H, W) -> out (N, C, Ho, Wo) with
 *   Ho = (H + 2 ph - kh) / sh + 1, Wo = (W + 2 pw - kw) / sw + 1 (integer division; both must be >= 1 and equal the Ho, Wo
 * passed in, -22 otherwise).  out[y][x] = the maximum over the window rows y sh - ph + i (i < kh) and columns x sw - pw + j
 * (j < kw) that lie inside the map, scanned row by row from -inf with ATen's rule `v > m || v != v`: padding behaves as
 * -inf, and a NaN in the window gives NaN.  kh, kw, sh, sw >= 1; 0 <= ph <= kh / 2, 0 <= pw <= kw / 2 (PyTorch's own limit).
 * One thread per output element.  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_maxpool_fwd(const float* in, int N, int C, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw,
                           float* out, int Ho, int Wo, tpspp_stream_t stream);

/*
 * The recurrent part of one bidirectional nn.LSTM layer with h_0 = c_0 = 0.
 *   xg   (T, N, 2, 4 hidden): x_t W_ih^T + (b_ih + b_hh) of direction d (0 forward, 1 reverse), PyTorch's gate order i, f, g, o
 *        (one tpspp_mm_f32 over all T N tokens and both directions);
 *   w_hh (2, 4 hidden, hidden): weight_hh_l0, weight_hh_l0_reverse as PyTorch stores them;
 *   out  (T, N, 2 hidden): the forward h_t at [..., :hidden], the reverse h_t at [..., hidden:].
 * Direction 0 visits t = 0 .. T-1, direction 1 visits t = T-1 .. 0.  Per step, image n and unit u, for each gate q:
 *   a_q = xg[t][n][d][q hidden + u] + sum_k h[n][k] w_hh[d][q hidden + u][k]
 * accumulated ON xg's value by v_mfma_f32_16x16x4_f32 (an fp32 fused multiply-add chain) in the fixed order
 * k = 16 b + 4 r + m for b = 0..15 (outer), m = 0..3, r = 0..3 (inner, one instruction); then
 *   c = sigma(a_f) c + sigma(a_i) tanh(a_g),   h = sigma(a_o) tanh(c)       (two multiplies and one add, not fused)
 *   sigma(x) = 1 / (1 + e) for x >= 0, e / (1 + e) for x < 0, with e = expf(-|x|) in (0, 1];
 *   tanh(x)  = copysign(-m / (m + 2), x) with m = expm1f(-2 |x|) in (-1, 0]:     neither can overflow for a finite x.
 * An image's output depends on its own xg rows alone: not on N, on its position in the batch or on images_per_group,
 * bit for bit.
 *
 * Work division: one workgroup of 512 threads owns one direction and one block of `images_per_group` images (rows of
 * the 16-row matrix-core tile; rows past the block stay zero) for all T steps: h in LDS (two copies of 16 x 256 floats,
 * swapped each step), c in registers, w_hh read again through L2 every step.  One workgroup barrier per step; no
 * communication between workgroups, no spin-wait, no grid barrier: every loop is bounded by T.
 * images_per_group: 0 lets the planner choose (tpspp_crnn_lstm_plan); accepted non-zero values: 4, 8, 16.
 * hidden must be TPSPP_CRNN_HIDDEN; T >= 1; T * N <= 2^30.  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_lstm_fwd(const float* xg, const float* w_hh, float* out, int T, int N, int hidden, int images_per_group,
                        tpspp_stream_t stream);

/*
 * The planner of tpspp_crnn_lstm_fwd, on the host: the images per workgroup it uses for a batch of N on a device with
 * `compute_units` CUs (<= 0: the current device's, 256 when there is none).  images_per_group != 0 is returned as it is
 * when accepted (-22 otherwise).  0: the largest g of 16, 8, 4 for which 2 * ceil(N / g) >= compute_units (every CU gets
 * a workgroup; a larger g reads w_hh less often per image), else 4.  The workgroup count is 2 * ceil(N / g).  N < 0: -22.
 */
int tpspp_crnn_lstm_plan(int N, int images_per_group, int compute_units);

/*
 * CTCConvertor.tensor2idx with topk = 1 on the device: logits (N, T, C) fp32, decode_len (N) int32 -> idx (N, T) int32,
 * score (N, T) fp32.  Per position: the arg-max class a_t (lowest index on equal maxima) and its softmax probability
 *   p_t = 1 / sum_c expf(l_c - max)     (64 lane-strided partial sums, classes ascending, then a butterfly over the lanes).
 * Position t is kept iff t < decode_len[n], a_t != blank and a_t != a_{t-1} (a_{-1} = blank): the scan of
 * convertors/ctc.py:119-129.  Kept positions get idx = a_t, score = p_t; every other position gets -1 and 0.
 * One wavefront per image.  C >= 2, 0 <= blank < C, T >= 1 (-22 otherwise).  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_ctc_decode(const float* logits, const int* decode_len, int N, int T, int C, int blank, int* idx,
                          float* score, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_CRNN_H_ */
