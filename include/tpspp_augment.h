/*
 * tpspp_augment.h -- the recogniser's TRAIN pipeline on the GPU (ABI 11): ResizeOCR, a per-image list of augmentation
 * ops, ToTensorOCR and NormalizeOCR in one launch, one workgroup per image, the uint8 image held in LDS from the resize to
 * the normalised store.
 *
 * A header of its own next to tpspp.h (whose types, return codes and conventions apply): device pointers, no allocation,
 * no host synchronisation, work enqueued on `stream`, 0 or a negative TPSPP_E* code with a message in tpspp_last_error();
 * every argument is checked before anything is launched.
 *
 * replaces: the per-image CPU work of configs/_base_/recog_pipelines/crnn_pp_pipeline.py:2-84 between ResizeOCR and
 *           NormalizeOCR -- TorchVisionWrapper(RandomAffine | RandomPerspective | ColorJitter), which transform_wrappers.py:
 *           113-123 runs on a PIL image (Image.transform(AFFINE, NEAREST), Image.transform(PERSPECTIVE, BILINEAR),
 *           ImageEnhance.Brightness / Contrast / Color, the hue shift through convert('HSV')), and RandomRotateTextDet
 *           (transforms.py:192-199, cv2.warpAffine(INTER_NEAREST)).  The random draws stay on the host: this entry point
 *           applies the op lists it is given.
 *
 * Op record: one int32 code and 8 doubles.  op_codes is (N, max_ops) int32, op_params (N, max_ops, 8) fp64, both in device
 * memory; image n runs its codes in order until the first code that is not one of 1..7 (0 ends the list; so does a code 6 or
 * 7 on a one-channel image).  Every op reads a uint8 image and writes a uint8 image of the same H x W x C; outside the
 * source a geometric op writes 0 (fill = 0).  "double" is IEEE fp64, "float" fp32, nothing is contracted.
 *
 *   1 TPSPP_AUG_AFFINE_NEAREST_PIL      params a0..a5, the inverse matrix.  Pillow's 16.16 fixed point: FIX(v) =
 *       (int)floor(v * 65536 + 0.5); xx = FIX(a2 + a0 * 0.5 + a1 * 0.5) + x * FIX(a0) + y * FIX(a1), yy likewise from a5, a3, a4
 *       (int32, wrapping); source (xx >> 16, yy >> 16), arithmetic shifts.                                        PINNED
 *   2 TPSPP_AUG_PERSPECTIVE_BILINEAR_PIL  params a0..a7.  xi = x + 0.5, yi = y + 0.5; xin = (a0 xi + a1 yi + a2) / (a6 xi +
 *       a7 yi + 1), yin from a3, a4, a5, in double; 0 unless 0 <= xin < W and 0 <= yin < H; then both minus 0.5, x0 = floor, dx =
 *       xin - x0; columns x0, x0 + 1 and row y0 clamped; v1 = p[xa] + (p[xb] - p[xa]) dx on row y0, v2 on row y0 + 1 if that row
 *       exists, else v1; (uint8)(v1 + (v2 - v1) dy), truncating.                                                   PINNED
 *   3 TPSPP_AUG_AFFINE_NEAREST_CV2      params M0..M5, the inverted 2x3 matrix.  OpenCV's warpAffine(INTER_NEAREST) in 10-bit
 *       fixed point: X = (rint(M0 x 1024) + rint((M1 y + M2) 1024) + 512) >> 10, Y from M3, M4, M5; constant border 0.
 *       UNPINNED: restated from OpenCV's published algorithm, never compared with OpenCV itself.
 *   4 TPSPP_AUG_BRIGHTNESS, 5 TPSPP_AUG_CONTRAST, 6 TPSPP_AUG_SATURATION   param f.  Pillow's blend of a degenerate image d
 *       with the image p: t = (float)d + (float)f * ((float)p - (float)d) in fp32; 0 <= f <= 1 stores (uint8)t, any other f
 *       clips t to 0..255 first.  d = 0 (brightness); the pixel's L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16 (saturation,
 *       three channels only); (int)(mean of L over the image + 0.5), the mean one double division of an exact integer sum
 *       (contrast).                                                                                                PINNED
 *   7 TPSPP_AUG_HUE                     param k = uint8(hue_factor * 255).  Pillow's RGB -> HSV, h += k modulo 256, HSV -> RGB;
 *       three channels only.                                                                                       PINNED
 *
 * PINNED = bit for bit against the installed Pillow's own outputs (tests/golden/augment_pillow.npz).
 */
#ifndef TPSPP_AUGMENT_H_
#define TPSPP_AUGMENT_H_

#include "tpspp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TPSPP_AUG_END                      0
#define TPSPP_AUG_AFFINE_NEAREST_PIL       1
#define TPSPP_AUG_PERSPECTIVE_BILINEAR_PIL 2
#define TPSPP_AUG_AFFINE_NEAREST_CV2       3
#define TPSPP_AUG_BRIGHTNESS               4
#define TPSPP_AUG_CONTRAST                 5
#define TPSPP_AUG_SATURATION               6
#define TPSPP_AUG_HUE                      7

#define TPSPP_AUG_MAX_OPS    8   /* op records per image */
#define TPSPP_AUG_OP_PARAMS  8   /* doubles per record */

/*
 * The first eleven arguments, `out` and `interpolation` are those of tpspp_resize_normalize_fwd, with the same meaning;
 * with every list empty the output has the same bits.  Limits of this entry point: C is 1 or 3; 1 <= max_ops <=
 * TPSPP_AUG_MAX_OPS; two H x W x C uint8 images must fit the 160 KB of LDS of a workgroup (-22 otherwise).
 * bgr: non-zero when channel 0 is blue (the order mmcv.imread gives and TorchVisionWrapper flips around its transform):
 * L and the hue arithmetic read R, G, B accordingly.
 * N == 0 returns 0 and launches nothing.
 */
int tpspp_augment_normalize_fwd(const unsigned char* src_packed, const long long* src_offsets,
                                const int* src_h, const int* src_w, const int* resize_w,
                                const float* lut, int pad_value, int N, int C, int H, int W,
                                float* out, int interpolation, const int* op_codes, const double* op_params,
                                int max_ops, int bgr, tpspp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* TPSPP_AUGMENT_H_ */
