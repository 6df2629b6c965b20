/*
 * tpspp_crnn_train.h -- the training kernels of the CRNN recogniser's recurrent half: what CRNNDecoder(rnn_flag=True)
 * and CTCLoss need, beyond tpspp.h and tpspp_crnn.h, to run forward and backward on this library
 * (CRNNDecoder.set_train_backend("hip"), CTCLoss.set_train_backend("hip")).
 *
 * tpspp.h's types, return codes and conventions apply: device pointers, no allocation, no host synchronisation, work
 * enqueued on `stream`, 0 or a negative TPSPP_E* code with a message in tpspp_last_error(); every argument is checked
 * before anything is launched.  TPSPP_ABI_VERSION is not raised by it: a library that lacks one of these symbols fails to
 * bind by name.
 *
 * replaces: the autograd of nn.LSTM(nIn, 256, bidirectional=True)'s recurrence      layers/lstm_layer.py:10,14
 *           torch.log_softmax + nn.CTCLoss, forward and backward                    losses/ctc_loss.py:50-71
 * The Linears around the recurrence (input projection, embedding) train on tpspp_mm_f32 and tpspp_linear_bwd_weight.
 *
 * "float" is IEEE fp32; nothing is contracted beyond the fused multiply-adds of the matrix cores.  No atomics: every
 * result is bitwise reproducible from call to call.
 */
#ifndef TPSPP_CRNN_TRAIN_H_
#define TPSPP_CRNN_TRAIN_H_

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * tpspp_crnn_lstm_fwd (tpspp_crnn.h: same operands, arithmetic, work division, planner and limits; `out` has the same
 * bits) that also stores, per step, image, direction d and unit u, what the backward reads:
 *   gates (T, N, 2, 4 hidden): sigma(a_i), sigma(a_f), tanh(a_g), sigma(a_o) at [t][n][d][q hidden + u], q = 0..3;
 *   cell  (T, N, 2, hidden):   c_t.
 * hidden must be 256; T >= 1; T * N <= 2^30; images_per_group 0, 4, 8 or 16.  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_lstm_train_fwd(const float* xg, const float* w_hh, float* out, float* gates, float* cell, int T, int N,
                              int hidden, int images_per_group, tpspp_stream_t stream);

/*
 * Backward through time of that recurrence: d_out (T, N, 2 hidden), the gradient of `out`, -> d_xg (T, N, 2, 4 hidden), the
 * gradient of the pre-activations a (a = xg + h W_hh^T, so of xg as well).  gates, cell: as the training forward stored
 * them.  w_hh_t (2, hidden, 4 hidden): w_hh of each direction transposed, w_hh_t[d][k][j] = w_hh[d][j][k].
 * d_xg_dir (2, T, N, 4 hidden) or NULL: the same values direction-major, d_xg_dir[d][t][n] = d_xg[t][n][d] -- dense rows per
 * direction, which is what tpspp_linear_bwd_weight takes as dy for d w_hh = sum_t da_t^T h_{t -+ 1}.
 * Each direction visits the steps in the reverse of its forward order, with dc = dh_rec = 0 before the first.  Per step,
 * image and unit (i, f, g, o = gates[t], c_prev = cell of the step the forward visited before, 0 at its first):
 *   dh = d_out[t] + dh_rec;   tc = tanh(cell[t]);   do = dh tc;   dc = dc + dh o (1 - tc tc)
 *   da_i = dc g i (1 - i);   da_f = dc c_prev f (1 - f);   da_g = dc i (1 - g g);   da_o = do o (1 - o)
 *   d_xg[t] = da (+ 0.0f: a zero is +0);   dc = dc f
 *   dh_rec[k] = sum_j da[j] w_hh[d][j][k], accumulated from 0 by v_mfma_f32_16x16x4_f32 in two chains, the even and the
 *   odd b of j = 16 b + 4 r + m, each in the fixed order b ascending (outer), m = 0..3, r = 0..3 (inner, one instruction),
 *   and added at the end (even + odd).
 * Every product above is an fp32 multiply evaluated left to right, tanh as in the forward (tpspp_crnn_lstm_fwd).  An image's
 * d_xg depends on its own rows alone: not on N, on its position in the batch or on images_per_group, bit for bit.
 *
 * Work division: the forward's.  One workgroup of 512 threads per direction and block of images for all T steps; the
 * forward's lane <-> (image, unit, four gates) mapping, so dc and dh_rec stay in registers; da in LDS (16 rows of 1024 + 4
 * floats, 64.25 KB: one workgroup per CU); w_hh_t read again through L2 every step.  Two workgroup barriers per step; no
 * communication between workgroups, no spin-wait, no grid barrier: every loop is bounded by T.
 * hidden must be 256; T >= 1; T * N <= 2^30; images_per_group 0 (the forward's planner), 4, 8 or 16.  N == 0 returns 0
 * and launches nothing.
 */
int tpspp_crnn_lstm_bwd(const float* d_out, const float* gates, const float* cell, const float* w_hh_t, float* d_xg,
                        float* d_xg_dir, int T, int N, int hidden, int images_per_group, tpspp_stream_t stream);

#define TPSPP_CTC_NONE 0
#define TPSPP_CTC_MEAN 1
#define TPSPP_CTC_SUM 2
#define TPSPP_CTC_MAX_CLASSES 1024
#define TPSPP_CTC_MAX_TARGET 1024

/*
 * Floats of workspace of the CTC loss: N * T * (2 Lmax + 1) for the alpha table, then N for each image's loss before
 * zero_infinity is applied (0 for N <= 0, T <= 0 or Lmax < 0).
 */
size_t tpspp_crnn_ctc_loss_workspace_floats(int N, int T, int Lmax);

/*
 * F.ctc_loss(log_softmax(logits, 2).permute(1, 0, 2), ...) from the raw logits: logits (N, T, C) fp32 dense, targets
 * (N, Lmax) int32 padded (read only when Lmax > 0), target_len and input_len (N) int32, clamped on the device to
 * 0 .. Lmax and 0 .. T (a target outside 0 .. C - 1 is clamped as well, so that nothing is read out of bounds; the caller
 * refuses such targets, and targets equal to blank).  No log-probability tensor exists:
 *   lse[n][t] = max_c x + log(sum_c exp(x_c - max)) for t < input_len (64 lane-strided partial sums, a butterfly), 0 after;
 *   lp_t(c) = x_c - lse[n][t].
 * Per image, over the S = 2 L + 1 extended states l' = (blank, l_1, blank, ..., l_L, blank), in log space:
 *   alpha_0(0) = lp_0(blank), alpha_0(1) = lp_0(l_1), -inf otherwise;
 *   alpha_t(s) = lp_t(l'_s) + LSE(alpha_{t-1}(s), alpha_{t-1}(s-1), and alpha_{t-1}(s-2) when l'_s != blank and
 *                l'_s != l'_{s-2})                                                      for 0 < t < input_len;
 *   loss_n = -LSE(alpha_last(S-1), alpha_last(S-2));   input_len = 0: 0 when L = 0, +inf otherwise.
 * LSE(a, b, ...) = m + log(exp(a - m) + exp(b - m) + ...) with m the maximum, and -inf when m = -inf: never NaN.
 * zero_infinity != 0: an infinite loss_n is replaced by 0.  ws keeps alpha (unused entries are -inf) and the loss_n before
 * that replacement; the backward reads both.
 * loss (N) always; reduction TPSPP_CTC_SUM: reduced[0] = sum_n loss_n; TPSPP_CTC_MEAN: reduced[0] = (sum_n loss_n /
 * max(L_n, 1)) / N (PyTorch's rule); both in one workgroup with a fixed order.  reduced may be NULL with TPSPP_CTC_NONE.
 * One wavefront per image, state s on lane s mod 64.
 * T >= 1, 2 <= C <= 1024, 0 <= blank < C, 0 <= Lmax <= 1024, N * T <= 2^30.  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_ctc_loss_fwd(const float* logits, const int* targets, const int* target_len, const int* input_len, int N,
                            int T, int C, int Lmax, int blank, int zero_infinity, int reduction, float* loss, float* lse,
                            float* reduced, float* ws, size_t ws_floats, tpspp_stream_t stream);

/*
 * Its backward: g (N) for TPSPP_CTC_NONE, (1) otherwise -> d_logits (N, T, C), every element written.  lse and ws are the
 * forward's.  With g_n = g[n] (none), g[0] (sum) or g[0] / (N max(L_n, 1)) (mean), beta recomputed backwards in time
 *   beta_last(S-1) = lp(blank), beta_last(S-2) = lp(l_L);
 *   beta_t(s) = lp_t(l'_s) + LSE(beta_{t+1}(s), beta_{t+1}(s+1), and beta_{t+1}(s+2) when l'_{s+2} != blank and
 *               l'_{s+2} != l'_s),
 *   d_logits[n][t][c] = g_n (exp(x_c - lse) - exp(LSE_{s: l'_s = c}(alpha_t(s) + beta_t(s)) - lp_t(c) + loss_n))
 * for t < input_len; rows t >= input_len are +0.  The per-class LSE takes the maximum, then adds exp(. - max) over the
 * states of that class in ascending s, by one lane: a character that occurs twice cannot make it order-dependent.
 * An image whose loss_n is +inf: with zero_infinity an all-zero block; without, its rows are unspecified (PyTorch's are
 * NaN) and no other image's rows are affected.
 * Limits as the forward's.  N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_ctc_loss_bwd(const float* g, const float* logits, const int* targets, const int* target_len,
                            const int* input_len, const float* lse, const float* ws, int N, int T, int C, int Lmax, int blank,
                            int zero_infinity, int reduction, float* d_logits, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_CRNN_TRAIN_H_ */
