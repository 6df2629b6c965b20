// GPU-side TRAIN pipeline of the recogniser: ResizeOCR -> per-image augmentation ops -> ToTensorOCR + NormalizeOCR in one
// launch (include/tpspp_augment.h holds the contract and the arithmetic of every op code).
//
// Reference: configs/_base_/recog_pipelines/crnn_pp_pipeline.py:2-84 -- RandomWrapper(OneOfWrapper[RandomRotateTextDet,
// TorchVisionWrapper(RandomAffine), TorchVisionWrapper(RandomPerspective)]) and RandomWrapper(TorchVisionWrapper(
// ColorJitter)) between ResizeOCR and ToTensorOCR.  TorchVisionWrapper turns the array into a PIL image
// (transform_wrappers.py:113-123), so the pixel work is Pillow's: Geometry.c (affine_fixed, perspective_transform +
// bilinear_filter8), Blend.c under ImageEnhance, Convert.c (rgb2l, rgb2hsv, hsv2rgb).  PINNED bit for bit against the
// installed Pillow (tests/golden/augment_pillow.npz).  RandomRotateTextDet is cv2.warpAffine(INTER_NEAREST)
// (transforms.py:192-199): PARITY UNPINNED, as the cv2 resize is.
//
// One workgroup per image.  The resized uint8 HWC image is written to LDS by the per-pixel functions the resize kernels use
// (tpspp_resize.h); every op reads one LDS image and writes the other (Pillow rounds to bytes between ops, and so does this),
// a workgroup barrier between ops; the last phase sends every byte through the (C, 256) table and stores plane by plane,
// consecutive lanes to consecutive floats.  The random draws are the host's (tps_pp_amd/ocr_transforms.py).
//
// Bound: HBM for empty lists (the bytes of tpspp_resize_normalize_fwd); with ops, LDS byte gathers and fp64 arithmetic
// (the perspective's two divisions per pixel, the HSV conversions), all of it on 12 KB per image.
#include "tpspp_augment.h"
#include "tpspp_common.h"
#include "tpspp_resize.h"

namespace {

// 16 wavefronts per image: a batch of 512 is only two workgroups per CU, and with 256 threads each the resize phase ran on
// two wavefronts per SIMD (empty lists: 22.5 us per 512 images against 20.7 with 1024, cv2 resize; 62.6 against 46.7, Pillow)
constexpr int kThreads = 1024;
constexpr int kLdsBytes = 160 * 1024;                          // per workgroup on gfx950

struct AugParams {
    const unsigned char* src;      // packed HWC images
    const long long* off;          // (N) byte offset of each image
    const int* sh; const int* sw;  // (N) source height / width
    const int* dw;                 // (N) resized width (<= W); columns >= dw[n] are padding
    const float* lut;              // (C, 256): value -> normalised float
    float* out;                    // (N, C, H, W)
    const int* codes;              // (N, max_ops)
    const double* params;          // (N, max_ops, 8)
    int N, H, W, pad_value, interpolation, max_ops, bgr;
    int img_bytes;                 // H * W * C rounded up to 16
};

__device__ __forceinline__ int fix16(double v) { return (int)floor(v * 65536.0 + 0.5); }
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's rgb2l
__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Pillow's ImagingBlend of a degenerate byte d with the image's byte p (fp32; `inside`: 0 <= f <= 1)
__device__ __forceinline__ unsigned char blend(int d, int p, float f, bool inside)
{
    float t = (float)d + f * ((float)p - (float)d);
    if (!inside) t = t <= 0.0f ? 0.0f : (t >= 255.0f ? 255.0f : t);
    return (unsigned char)(int)t;
}

// Pillow's rgb2hsv, h += k (mod 256), hsv2rgb
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int k)
{
    const int maxc = max(max(r, g), b), minc = min(min(r, g), b);
    int uh = 0, us = 0;
    const int uv = maxc;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
        float h;
        if (r == maxc) h = (float)((double)bc - (double)gc);
        else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double x = (double)h / 6.0 + 1.0;                 // > 0: fmod(x, 1.0) = x - floor(x), exactly
        h = (float)(x - floor(x));
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + k) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double hf = (double)uh * 6.0 / 255.0;
    const double fi = floor(hf);
    const double f = (double)(float)(hf - fi);
    const double fs = (double)(float)((double)us / 255.0);
    const double v = (double)uv;
    const int p = clip8((int)floor(v * (1.0 - fs) + 0.5));
    const int q = clip8((int)floor(v * (1.0 - fs * f) + 0.5));
    const int t = clip8((int)floor(v * (1.0 - fs * (1.0 - f)) + 0.5));
    switch ((int)fi % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
    }
}

template <int C>
__global__ void __launch_bounds__(kThreads)
augment_norm_kernel(const AugParams P)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned char* cur = smem;
    unsigned char* nxt = smem + P.img_bytes;
    unsigned int* red = reinterpret_cast<unsigned int*>(smem + 2 * (size_t)P.img_bytes);
    const int n = blockIdx.x, tid = threadIdx.x;
    const int H = P.H, W = P.W, HW = H * W;
    const int ir = P.bgr ? 2 : 0, ib = P.bgr ? 0 : 2;          // where R and B sit in a three-channel pixel

    // ---- 1. ResizeOCR into LDS ---------------------------------------------------------------------------------------
    {
        const int SH = P.sh[n], SW = P.sw[n], DW = P.dw[n];
        const unsigned char* img = P.src + P.off[n];
        for (int p = tid; p < HW; p += kThreads) {
            const int y = p / W, x = p - y * W;
            unsigned char* d = cur + p * C;
            auto store = [&](int c, int v) { d[c] = (unsigned char)v; };
            if (x >= DW) {                                     // mmcv.impad: constant padding on the right
#pragma unroll
                for (int c = 0; c < C; ++c) d[c] = (unsigned char)P.pad_value;
            } else if (P.interpolation == TPSPP_RESIZE_PILLOW) {
                tpspp::resize::pillow_pixel<C>(img, SH, SW, DW, H, x, y, store);
            } else {
                tpspp::resize::cv2_pixel(img, SH, SW, DW, H, C, x, y, store);
            }
        }
    }
    __syncthreads();

    // ---- 2. the image's op list: cur -> nxt, swap ----------------------------------------------------------------------
    for (int k = 0; k < P.max_ops; ++k) {
        const int code = P.codes[(size_t)n * P.max_ops + k];   // the same word for every thread: the barriers below are uniform
        if (code < TPSPP_AUG_AFFINE_NEAREST_PIL || code > TPSPP_AUG_HUE || (C == 1 && code >= TPSPP_AUG_SATURATION)) break;
        const double* a = P.params + ((size_t)n * P.max_ops + k) * TPSPP_AUG_OP_PARAMS;
        if (code == TPSPP_AUG_AFFINE_NEAREST_PIL) {
            // unsigned arithmetic: the wrap-around of Pillow's accumulating int, without signed overflow
            const unsigned sxx = (unsigned)fix16(a[0]), sxy = (unsigned)fix16(a[1]);
            const unsigned syx = (unsigned)fix16(a[3]), syy = (unsigned)fix16(a[4]);
            const unsigned ox = (unsigned)fix16(a[2] + a[0] * 0.5 + a[1] * 0.5);
            const unsigned oy = (unsigned)fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
            for (int p = tid; p < HW; p += kThreads) {
                const int y = p / W, x = p - y * W;
                const int xin = (int)(ox + (unsigned)x * sxx + (unsigned)y * sxy) >> 16;
                const int yin = (int)(oy + (unsigned)x * syx + (unsigned)y * syy) >> 16;
                const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
                const unsigned char* s = cur + (ok ? (yin * W + xin) * C : 0);
#pragma unroll
                for (int c = 0; c < C; ++c) nxt[p * C + c] = ok ? s[c] : (unsigned char)0;
            }
        } else if (code == TPSPP_AUG_AFFINE_NEAREST_CV2) {
            const double m0 = a[0], m1 = a[1], m2 = a[2], m3 = a[3], m4 = a[4], m5 = a[5];
            for (int p = tid; p < HW; p += kThreads) {
                const int y = p / W, x = p - y * W;
                const long long X = ((long long)(int)rint(m0 * (double)x * 1024.0) + (int)rint((m1 * (double)y + m2) * 1024.0) + 512) >> 10;
                const long long Y = ((long long)(int)rint(m3 * (double)x * 1024.0) + (int)rint((m4 * (double)y + m5) * 1024.0) + 512) >> 10;
                const bool ok = X >= 0 && X < W && Y >= 0 && Y < H;
                const unsigned char* s = cur + (ok ? ((int)Y * W + (int)X) * C : 0);
#pragma unroll
                for (int c = 0; c < C; ++c) nxt[p * C + c] = ok ? s[c] : (unsigned char)0;
            }
        } else if (code == TPSPP_AUG_PERSPECTIVE_BILINEAR_PIL) {
            const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7];
            for (int p = tid; p < HW; p += kThreads) {
                const int y = p / W, x = p - y * W;
                const double xi = (double)x + 0.5, yi = (double)y + 0.5;
                const double den = a6 * xi + a7 * yi + 1.0;
                double xin = (a0 * xi + a1 * yi + a2) / den;
                double yin = (a3 * xi + a4 * yi + a5) / den;
                // (a NaN coordinate passes Pillow's test as well; its floor below is clamped like any other)
                const bool outside = xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H;
                xin -= 0.5;
                yin -= 0.5;
                const double fx = floor(xin), fy = floor(yin);
                const double dx = xin - fx, dy = yin - fy;
                const int x0 = min(max((int)fx, -1), W), y0 = min(max((int)fy, -1), H);   // (beyond: outside, or clamped alike)
                const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
                const unsigned char* r0 = cur + min(max(y0, 0), H - 1) * W * C;
                const bool has = y0 + 1 >= 0 && y0 + 1 < H;
                const unsigned char* r1 = cur + (has ? y0 + 1 : 0) * W * C;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double p00 = (double)r0[xa * C + c], p01 = (double)r0[xb * C + c];
                    const double v1 = p00 + (p01 - p00) * dx;
                    double v2 = v1;
                    if (has) {
                        const double p10 = (double)r1[xa * C + c], p11 = (double)r1[xb * C + c];
                        v2 = p10 + (p11 - p10) * dx;
                    }
                    const double v = v1 + (v2 - v1) * dy;
                    nxt[p * C + c] = outside ? (unsigned char)0 : (unsigned char)(int)v;
                }
            }
        } else if (code == TPSPP_AUG_BRIGHTNESS) {
            const float f = (float)a[0];
            const bool inside = f >= 0.0f && f <= 1.0f;
            for (int i = tid; i < HW * C; i += kThreads) nxt[i] = blend(0, cur[i], f, inside);
        } else if (code == TPSPP_AUG_CONTRAST) {
            const float f = (float)a[0];
            const bool inside = f >= 0.0f && f <= 1.0f;
            if (tid == 0) *red = 0u;
            __syncthreads();
            unsigned int sum = 0u;                             // exact: at most 255 * 81920 pixels
            for (int p = tid; p < HW; p += kThreads)
                sum += C == 1 ? (unsigned)cur[p] : (unsigned)luma(cur[p * C + ir], cur[p * C + 1], cur[p * C + ib]);
            atomicAdd(red, sum);                               // integer: the order does not matter
            __syncthreads();
            const int mean = (int)((double)*red / (double)HW + 0.5);
            for (int i = tid; i < HW * C; i += kThreads) nxt[i] = blend(mean, cur[i], f, inside);
        } else if (code == TPSPP_AUG_SATURATION) {
            const float f = (float)a[0];
            const bool inside = f >= 0.0f && f <= 1.0f;
            for (int p = tid; p < HW; p += kThreads) {
                const int L = luma(cur[p * C + ir], cur[p * C + 1], cur[p * C + ib]);
#pragma unroll
                for (int c = 0; c < C; ++c) nxt[p * C + c] = blend(L, cur[p * C + c], f, inside);
            }
        } else {                                               // TPSPP_AUG_HUE
            const int kk = (int)a[0] & 255;
            for (int p = tid; p < HW; p += kThreads) {
                int r = cur[p * C + ir], g = cur[p * C + 1], b = cur[p * C + ib];
                hue_shift(r, g, b, kk);
                nxt[p * C + ir] = (unsigned char)r;
                nxt[p * C + 1] = (unsigned char)g;
                nxt[p * C + ib] = (unsigned char)b;
            }
        }
        __syncthreads();
        unsigned char* t = cur; cur = nxt; nxt = t;
    }

    // ---- 3. ToTensorOCR + NormalizeOCR: table lookup, plane-wise stores -------------------------------------------------
    float* o = P.out + (size_t)n * C * HW;
#pragma unroll
    for (int c = 0; c < C; ++c)
        for (int p = tid; p < HW; p += kThreads) o[(size_t)c * HW + p] = P.lut[c * 256 + cur[p * C + c]];
}

}  // namespace

TPSPP_EXPORT int tpspp_augment_normalize_fwd(const unsigned char* src_packed, const long long* src_offsets,
                                             const int* src_h, const int* src_w, const int* resize_w,
                                             const float* lut, int pad_value, int N, int C, int H, int W,
                                             float* out, int interpolation, const int* op_codes, const double* op_params,
                                             int max_ops, int bgr, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(interpolation == TPSPP_RESIZE_CV2 || interpolation == TPSPP_RESIZE_PILLOW,
                  "tpspp_augment_normalize_fwd: interpolation must be TPSPP_RESIZE_CV2 (0) or TPSPP_RESIZE_PILLOW (1)");
    TPSPP_REQUIRE(src_packed && src_offsets && src_h && src_w && resize_w && lut && out && op_codes && op_params,
                  "tpspp_augment_normalize_fwd: null pointer");
    TPSPP_REQUIRE(N >= 0 && (C == 1 || C == 3) && H > 0 && W > 0 && pad_value >= 0 && pad_value <= 255,
                  "tpspp_augment_normalize_fwd: bad sizes (1 or 3 channels, pad value 0..255)");
    TPSPP_REQUIRE(max_ops >= 1 && max_ops <= TPSPP_AUG_MAX_OPS,
                  "tpspp_augment_normalize_fwd: max_ops must be 1..%d", TPSPP_AUG_MAX_OPS);
    const long long img_bytes = ((long long)H * W * C + 15) / 16 * 16;
    const long long lds = 2 * img_bytes + 16;                  // two images and the contrast sum
    TPSPP_REQUIRE(lds <= kLdsBytes,
                  "tpspp_augment_normalize_fwd: two %d x %d x %d uint8 images (%lld bytes) do not fit the LDS (%d bytes)",
                  H, W, C, lds, kLdsBytes);
    if (N == 0) return TPSPP_OK;
    AugParams P;
    P.src = src_packed; P.off = src_offsets; P.sh = src_h; P.sw = src_w; P.dw = resize_w; P.lut = lut; P.out = out;
    P.codes = op_codes; P.params = op_params;
    P.N = N; P.H = H; P.W = W; P.pad_value = pad_value; P.interpolation = interpolation; P.max_ops = max_ops;
    P.bgr = bgr ? 1 : 0; P.img_bytes = (int)img_bytes;
    static bool attr_done[tpspp::kMaxDevices] = {};
    if (tpspp::first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&augment_norm_kernel<1>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&augment_norm_kernel<3>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        (void)hipGetLastError();
    }
    hipStream_t st = tpspp::as_stream(stream);
    if (C == 1)
        hipLaunchKernelGGL(augment_norm_kernel<1>, dim3((unsigned)N), dim3(kThreads), (size_t)lds, st, P);
    else
        hipLaunchKernelGGL(augment_norm_kernel<3>, dim3((unsigned)N), dim3(kThreads), (size_t)lds, st, P);
    return tpspp::check_launch("tpspp_augment_normalize_fwd");
}
