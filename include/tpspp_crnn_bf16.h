/*
 * tpspp_crnn_bf16.h -- what VeryDeepVgg needs, beyond tpspp.h and tpspp_crnn.h, to run in the reduced-precision
 * configurations (compute_dtype "bf16x3" or torch.bfloat16): its max-pools on the blocked layouts the bf16 convolutions
 * (tpspp_conv2d_bf16_fwd) exchange, so that the feature maps stay blocked from conv0's output to conv6's input.
 *
 * tpspp.h's types, return codes and conventions apply: device pointers, no allocation, no host synchronisation, work
 * enqueued on `stream`, 0 or a negative TPSPP_E* code with a message in tpspp_last_error(); every argument is checked
 * before anything is launched.  TPSPP_ABI_VERSION is not raised by it: a library that lacks one of these symbols fails to
 * bind by name.
 *
 * replaces: nn.MaxPool2d(2, 2) and nn.MaxPool2d((2, 2), (2, 1), (0, 1))     backbones/very_deep_vgg.py:51-60
 * when the module runs in a reduced mode.  The convolutions of those modes are tpspp_conv2d_bf16_fwd (tpspp.h).
 */
#ifndef TPSPP_CRNN_BF16_H_
#define TPSPP_CRNN_BF16_H_

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * tpspp_crnn_maxpool_fwd (tpspp_crnn.h) on a blocked map: in (N, C / 8, H, W, 8) -> out (N, C / 8, Ho, Wo, 8), the eight
 * channels of a group next to each other per pixel.  `layout` is tpspp_conv2d_bf16_fwd's code: 2 bf16, 3 fp32; `out` has
 * the layout of `in`.  C must be a multiple of 8; both pointers 16-byte aligned.
 *   Ho = (H + 2 ph - kh) / sh + 1, Wo = (W + 2 pw - kw) / sw + 1 (integer division; both must be >= 1 and equal the Ho, Wo
 * passed in, -22 otherwise).  Per channel, out[y][x] = the maximum over the window rows y sh - ph + i (i < kh) and columns
 * x sw - pw + j (j < kw) that lie inside the map, scanned row by row from -inf with ATen's rule `v > m || v != v`: padding
 * behaves as -inf, and a NaN in the window gives NaN.  bf16 values are widened to fp32 for the comparison, which is exact:
 * the result is one of the inputs, and has the bits F.max_pool2d gives on the NCHW view in both layouts.
 * kh, kw, sh, sw >= 1; 0 <= ph <= kh / 2, 0 <= pw <= kw / 2 (PyTorch's own limit).
 * One thread per (image, channel group, output pixel), neighbouring lanes on neighbouring output columns; per window
 * position one 16-byte load (bf16) or two (fp32), and as many 16-byte stores per output.  No LDS, no atomics.
 * N == 0 returns 0 and launches nothing.
 */
int tpspp_crnn_maxpool_blk_fwd(const void* in, int layout, int N, int C, int H, int W, int kh, int kw, int sh, int sw,
                               int ph, int pw, void* out, int Ho, int Wo, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_CRNN_BF16_H_ */
