/*
 * tpspp_train_opt.h -- the last stage of a training iteration: one multi-tensor Adam / AdamW update of every parameter
 * in one launch, the L2 norm of all gradients with its clipping coefficient (never read by the host), and a one-launch
 * zeroing of all gradients.  Exact fp32, IEEE square root and division, no fast-math.
 *
 * A header of its own next to tpspp.h, tpspp_train_attn.h and tpspp_train_dec.h (whose types, return codes and
 * conventions apply): device pointers, no allocation, no host synchronisation, work enqueued on `stream`, 0 or a negative
 * TPSPP_E* code with a message in tpspp_last_error(); every argument is checked before anything is launched.
 *
 * replaces: the single-tensor arithmetic of torch.optim.Adam / torch.optim.AdamW (amsgrad=False, maximize=False), one
 *           launch for all parameters instead of several per parameter; torch.nn.utils.clip_grad_norm_ (norm_type 2; the
 *           gradients are NOT scaled in place: the coefficient goes to the update by device pointer); the backward-clip-step
 *           sequence of mmcv's OptimizerHook (optimizer_config.grad_clip), of which these entry points are the clip and the
 *           step.
 *
 * Fixed summation orders, no float atomics: every entry point is bitwise reproducible from call to call, and an element's
 * update does not depend on which other tensors share the launch.
 *
 * Operands: pointers do not travel as kernel arguments (390 tensors x 4 would not fit); three arrays in DEVICE memory,
 * built by the caller, describe the work:
 *   table     (n_tensors, 5) int64, row t = { address of p, of g, of m, of v, element count }.  fp32 tensors, dense,
 *             4-byte aligned at least; count >= 1.  tpspp_mt_sumsq and tpspp_mt_zero read columns 1 and 4 only.
 *   scalars   (n_tensors, 4) fp32, row t = { step_size, bc2_sqrt, wd, decay }, computed by the caller in double and
 *             rounded once:  step_size = lr / (1 - beta1^t),  bc2_sqrt = sqrt(1 - beta2^t),  wd = the weight decay,
 *             decay = 1 - lr * wd (read in AdamW mode only).
 *   chunk_map (n_chunks, 2) int64, row c = { tensor index, first element }: workgroup c works on the elements
 *             [first, min(first + chunk, count)) of that tensor.  A row that names no tensor of the table, or a first
 *             element outside its tensor, makes its workgroup do nothing.
 * chunk: elements per workgroup, a positive multiple of 4 (the vector width), at most 2^20.  threads: the workgroup size,
 * one of 64, 128, 256, 512, 1024.  Thread i of a workgroup owns the elements 4i .. 4i+3 of every slice of 4 * threads
 * elements of its chunk, on both of the paths below, so results do not depend on the path.
 * Alignment is decided per chunk from the addresses: where p, g, m and v at the chunk's first element are all 16-byte
 * aligned, whole groups of four move as 128-bit loads and stores; a chunk of a tensor that starts at an odd element offset
 * of its storage, and the last one to three elements of a tensor, move element by element.
 */
#ifndef TPSPP_TRAIN_OPT_H_
#define TPSPP_TRAIN_OPT_H_

#include <stddef.h>

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TPSPP_OPT_ADAM  0   /* weight decay joins the gradient: g' += wd * p */
#define TPSPP_OPT_ADAMW 1   /* decoupled weight decay: p *= decay */

/*
 * Per element, with c = coef[0] (coef == NULL: the gradient is taken as it is) and the tensor's scalar row:
 *     g' = c * g                                            one rounding
 *     Adam,  wd != 0:   g' = fma(wd, p, g')                 fused
 *     AdamW:            p  = p * decay                      one rounding
 *     m = fma(1 - beta1, g' - m, m)                         g' - m rounded, then fused (torch's lerp form)
 *     v = fma((1 - beta2) * g', g', beta2 * v)              both inner products rounded, then fused
 *     p = fma(-step_size, m / (sqrt(v) / bc2_sqrt + eps), p)    sqrt, both divisions and the sum rounded, then fused
 * beta1, beta2 and eps travel in double: beta2, 1 - beta1, 1 - beta2 and eps are each rounded to fp32 once, as PyTorch rounds
 * its Python scalars (1 - (float)0.999 would be off by 1.3e-5 of itself).  g is read and never written.  step_size == 0 (lr == 0)
 * leaves p bit-unchanged while m and v advance; g == m == v == 0 leaves p bit-unchanged and m, v at +0.0.
 * Limits: 0 <= beta1, beta2 < 1, eps >= 0 and finite.
 */
int tpspp_mt_adam(const long long* table, const float* scalars, int n_tensors, const long long* chunk_map, int n_chunks,
                  int chunk, int threads, double beta1, double beta2, double eps, int mode, const float* coef,
                  tpspp_stream_t stream);

/*
 * partials[c] = the sum of g^2 over chunk c in fp32: every thread adds its elements ascending with fma(g, g, acc), the 64
 * lanes of a wavefront combine in a fixed butterfly order, the wavefronts ascending.  partials: n_chunks floats
 * (partial_floats >= n_chunks is checked).
 */
int tpspp_mt_sumsq(const long long* table, int n_tensors, const long long* chunk_map, int n_chunks, int chunk, int threads,
                   float* partials, size_t partial_floats, tpspp_stream_t stream);

/*
 * One workgroup of 256 threads adds the partials in index order in fp64 (thread i the i-th contiguous run of
 * ceil(n_chunks / 256) partials, then the 256 sums ascending) and writes out[0..2] (fp32):
 *     out[0] = norm = sqrt(sum),  out[1] = coef = min(1, max_norm / (norm + 1e-6)) (NaN if the norm is),
 *     out[2] = 1 if the norm is not finite, else 0.
 * max_norm > 0.
 */
int tpspp_mt_norm_finish(const float* partials, int n_chunks, float max_norm, float* out, tpspp_stream_t stream);

/* Writes +0.0 over every gradient of the table. */
int tpspp_mt_zero(const long long* table, int n_tensors, const long long* chunk_map, int n_chunks, int chunk, int threads,
                  tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_TRAIN_OPT_H_ */
