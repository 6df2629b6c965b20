// Per-pixel arithmetic of ResizeOCR's two backends, shared by tpspp_resize.hip (one thread per output pixel, straight to
// the normalised fp32 tensor) and tpspp_augment.hip (the resized uint8 image goes to LDS first).  Each function computes
// the C bytes of ONE output pixel (x, y) of an image resized SH x SW -> H x DW and hands them to `store(c, value)`; what
// the arithmetic restates, and which half of it is pinned, is written at the top of tpspp_resize.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace tpspp {
namespace resize {

__device__ __forceinline__ void coeff(int d, int src, int dst, int& s, float& f)
{
    const double scale = 1.0 / ((double)dst / (double)src);
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f = f - (float)s;
}

__device__ __forceinline__ int sat_short(float v)
{
    const float r = rintf(v);                                  // cvRound: nearest, ties to even
    return (int)fminf(fmaxf(r, -32768.0f), 32767.0f);
}

// OpenCV's 8-bit INTER_LINEAR (INTER_AREA for an exact 2x2 shrink); x < DW
template <class Store>
__device__ __forceinline__ void cv2_pixel(const unsigned char* img, int SH, int SW, int DW, int H, int C, int x, int y,
                                          Store store)
{
    if (SH == 2 * H && SW == 2 * DW) {                         // INTER_AREA, exact 2x2
        const unsigned char* r0 = img + ((size_t)(2 * y) * SW + 2 * x) * C;
        const unsigned char* r1 = r0 + (size_t)SW * C;
        for (int c = 0; c < C; ++c)
            store(c, ((int)r0[c] + (int)r0[C + c] + (int)r1[c] + (int)r1[C + c] + 2) >> 2);
        return;
    }
    int sx, sy;
    float fx, fy;
    coeff(x, SW, DW, sx, fx);
    coeff(y, SH, H, sy, fy);
    if (sx < 0) { fx = 0.0f; sx = 0; }
    if (sx >= SW - 1) { fx = 0.0f; sx = SW - 1; }
    const int a0 = sat_short((1.0f - fx) * 2048.0f), a1 = sat_short(fx * 2048.0f);
    const int b0 = sat_short((1.0f - fy) * 2048.0f), b1 = sat_short(fy * 2048.0f);
    const int sx1 = min(sx + 1, SW - 1);
    const int y0 = min(max(sy, 0), SH - 1), y1 = min(max(sy + 1, 0), SH - 1);
    const unsigned char* r0 = img + (size_t)y0 * SW * C;
    const unsigned char* r1 = img + (size_t)y1 * SW * C;
    for (int c = 0; c < C; ++c) {
        const int S0 = (int)r0[sx * C + c] * a0 + (int)r0[sx1 * C + c] * a1;
        const int S1 = (int)r1[sx * C + c] * a0 + (int)r1[sx1 * C + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        store(c, min(max(v, 0), 255));
    }
}

// ---- Pillow's BILINEAR (Resample.c) --------------------------------------------------------------------------------------
struct PilAxis { int lo, n; double center, ss, ww; };

__device__ __forceinline__ double pil_triangle(double x)
{
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// precompute_coeffs for ONE output index d of an axis resampled in_size -> out_size (box = the whole image)
__device__ __forceinline__ PilAxis pil_axis(int d, int in_size, int out_size)
{
    PilAxis A;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;                 // bilinear: support 1.0
    A.ss = 1.0 / filterscale;
    A.center = ((double)d + 0.5) * scale;
    int lo = (int)(A.center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(A.center + support + 0.5);
    if (hi > in_size) hi = in_size;
    A.lo = lo;
    A.n = hi - lo;
    double ww = 0.0;
    for (int x = 0; x < A.n; ++x) ww += pil_triangle(((double)(x + lo) - A.center + 0.5) * A.ss);
    A.ww = ww;
    return A;
}

// k[x] / ww, then normalize_coeffs_8bpc
__device__ __forceinline__ int pil_coef(const PilAxis& A, int x)
{
    double w = pil_triangle(((double)(x + A.lo) - A.center + 0.5) * A.ss);
    if (A.ww != 0.0) w = w / A.ww;
    return w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
}

__device__ __forceinline__ int pil_clip8(int v)
{
    v >>= 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Pillow's two passes for one output pixel; x < DW
// (an axis that is not resized has the coefficients {2^22} / {2^22, 0}: the pass Pillow skips is an exact identity here)
template <int C, class Store>
__device__ __forceinline__ void pillow_pixel(const unsigned char* img, int SH, int SW, int DW, int H, int x, int y,
                                             Store store)
{
    const PilAxis AX = pil_axis(x, SW, DW), AY = pil_axis(y, SH, H);
    constexpr int KC = 8;                                      // horizontal coefficients kept in registers (scale <= 3.5)
    int kx[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) kx[j] = j < AX.n ? pil_coef(AX, j) : 0;
    int vacc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) vacc[c] = 1 << 21;
    for (int i = 0; i < AY.n; ++i) {
        const int ky = pil_coef(AY, i);
        const unsigned char* row = img + ((size_t)(AY.lo + i) * SW + AX.lo) * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
        if (AX.n <= KC) {
#pragma unroll
            for (int j = 0; j < KC; ++j)
                if (j < AX.n) {
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c] += (int)row[j * C + c] * kx[j];
                }
        } else {
            for (int j = 0; j < AX.n; ++j) {
                const int k = pil_coef(AX, j);
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)row[j * C + c] * k;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) vacc[c] += pil_clip8(acc[c]) * ky;          // the horizontal pass's uint8 image, times ky
    }
#pragma unroll
    for (int c = 0; c < C; ++c) store(c, pil_clip8(vacc[c]));
}

}  // namespace resize
}  // namespace tpspp
