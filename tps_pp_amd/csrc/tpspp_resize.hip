// GPU-side ResizeOCR + ToTensorOCR + NormalizeOCR: a batch of uint8 HWC crops of
// different sizes -> one (N, C, H, W_max) fp32 tensor, resized (bilinear), right-padded and normalised, so that the
// recogniser's input no longer passes through a CPU data loader.
//
// Reference: mmocr/datasets/pipelines/ocr_transforms.py:67-156 (ResizeOCR.__call__, ToTensorOCR, NormalizeOCR) as
// configured by configs/_base_/recog_pipelines/crnn_pp_pipeline.py:85-95.  The resize there is mmcv.imresize ->
// cv::resize(INTER_LINEAR) on uint8; this kernel follows OpenCV's published 8-bit algorithm (resize.cpp: source
// coordinate from a double scale cast to float, 11-bit fixed-point weights rounded to nearest-even, horizontal pass in
// int32, vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2; INTER_AREA for an exact 2x2 shrink).
// PARITY UNPINNED: OpenCV is not installed where this was built, so the integer arithmetic is checked bit-for-bit
// against oracle/resize_oracle.py (the same restatement) and not against OpenCV itself.  "/255, -mean, /std" is a
// 256-entry table per channel computed by the caller with torch's own fp32 arithmetic, hence exact.
//
// Round 6 -- interpolation 1 = backend='pillow' (ocr_transforms.py:46,65,99-101 forward `backend` to mmcv.imresize, whose
// pillow branch is Image.fromarray(img).resize(size, Image.BILINEAR)): resize_norm_pillow_kernel restates Pillow's
// src/libImaging/Resample.c -- precompute_coeffs in double (support = max(scale, 1), window [int(center - support + 0.5),
// int(center + support + 0.5)) clipped to the image, triangle weights normalised by their ascending sum),
// normalize_coeffs_8bpc (int(0.5 + k 2^22)), horizontal pass into uint8, then the vertical pass, each
// clip8((2^21 + sum(pixel * k)) >> 22).  IEEE double +, -, *, / with -ffp-contract=off are the same operations on the device as
// in Pillow's C on the host, so the coefficients are computed where they are used.  PINNED: tests/golden/resize_pillow.npz
// holds the installed Pillow's own outputs (tests/golden/make_resize_golden.py) and the -m gpu test compares bit for bit.
//
// Bound: HBM, trivially (one thread per output pixel: 4 taps x C bytes in, C floats out; 49 KB per 32x128 image).
#include "tpspp_common.h"
#include "tpspp_resize.h"   // the per-pixel arithmetic, shared with tpspp_augment.hip

namespace {

struct ResizeParams {
    const unsigned char* src;      // packed HWC images
    const long long* off;          // (N) byte offset of each image
    const int* sh; const int* sw;  // (N) source height / width
    const int* dw;                 // (N) resized width (<= W); columns >= dw[n] are padding
    const float* lut;              // (C, 256): value -> normalised float
    float* out;                    // (N, C, H, W)
    int N, C, H, W, pad_value;
};

__global__ void __launch_bounds__(256)
resize_norm_kernel(const ResizeParams P)
{
    const int n = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.H * P.W) return;
    const int y = p / P.W, x = p - y * P.W;
    const int SH = P.sh[n], SW = P.sw[n], DW = P.dw[n], C = P.C;
    const unsigned char* img = P.src + P.off[n];
    float* o = P.out + ((size_t)n * C * P.H + y) * P.W + x;
    const size_t plane = (size_t)P.H * P.W;
    if (x >= DW) {                                             // mmcv.impad: constant padding on the right
        for (int c = 0; c < C; ++c) o[c * plane] = P.lut[c * 256 + P.pad_value];
        return;
    }
    tpspp::resize::cv2_pixel(img, SH, SW, DW, P.H, C, x, y, [&](int c, int v) { o[c * plane] = P.lut[c * 256 + v]; });
}

template <int C>
__global__ void __launch_bounds__(256)
resize_norm_pillow_kernel(const ResizeParams P)
{
    const int n = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P.H * P.W) return;
    const int y = p / P.W, x = p - y * P.W;
    const int SH = P.sh[n], SW = P.sw[n], DW = P.dw[n];
    const unsigned char* img = P.src + P.off[n];
    float* o = P.out + ((size_t)n * C * P.H + y) * P.W + x;
    const size_t plane = (size_t)P.H * P.W;
    if (x >= DW) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c * plane] = P.lut[c * 256 + P.pad_value];
        return;
    }
    tpspp::resize::pillow_pixel<C>(img, SH, SW, DW, P.H, x, y, [&](int c, int v) { o[c * plane] = P.lut[c * 256 + v]; });
}

}  // namespace

TPSPP_EXPORT int tpspp_resize_normalize_fwd(const unsigned char* src_packed, const long long* src_offsets,
                                            const int* src_h, const int* src_w, const int* resize_w,
                                            const float* lut, int pad_value, int N, int C, int H, int W,
                                            float* out, int interpolation, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(interpolation == TPSPP_RESIZE_CV2 || interpolation == TPSPP_RESIZE_PILLOW,
                  "tpspp_resize_normalize_fwd: interpolation must be TPSPP_RESIZE_CV2 (0) or TPSPP_RESIZE_PILLOW (1)");
    TPSPP_REQUIRE(src_packed && src_offsets && src_h && src_w && resize_w && lut && out,
                  "tpspp_resize_normalize_fwd: null pointer");
    TPSPP_REQUIRE(N >= 0 && C >= 1 && C <= 4 && H > 0 && W > 0 && pad_value >= 0 && pad_value <= 255,
                  "tpspp_resize_normalize_fwd: bad sizes (1..4 channels, pad value 0..255)");
    TPSPP_REQUIRE(N <= 65535, "tpspp_resize_normalize_fwd: at most 65535 images per call");
    if (N == 0) return TPSPP_OK;
    ResizeParams P;
    P.src = src_packed; P.off = src_offsets; P.sh = src_h; P.sw = src_w; P.dw = resize_w; P.lut = lut; P.out = out;
    P.N = N; P.C = C; P.H = H; P.W = W; P.pad_value = pad_value;
    const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)N);
    hipStream_t st = tpspp::as_stream(stream);
    if (interpolation == TPSPP_RESIZE_PILLOW) {
        switch (C) {
        case 1: hipLaunchKernelGGL(resize_norm_pillow_kernel<1>, grid, dim3(256), 0, st, P); break;
        case 2: hipLaunchKernelGGL(resize_norm_pillow_kernel<2>, grid, dim3(256), 0, st, P); break;
        case 3: hipLaunchKernelGGL(resize_norm_pillow_kernel<3>, grid, dim3(256), 0, st, P); break;
        default: hipLaunchKernelGGL(resize_norm_pillow_kernel<4>, grid, dim3(256), 0, st, P); break;
        }
    } else {
        hipLaunchKernelGGL(resize_norm_kernel, grid, dim3(256), 0, st, P);
    }
    return tpspp::check_launch("tpspp_resize_normalize_fwd");
}
