// The backward of nn.MaxPool2d with the in-place ReLU's backward folded in (include/tpspp.h: tpspp_crnn_maxpool_bwd): the one
// kernel VeryDeepVgg's training graph lacked (VeryDeepVgg.set_vgg_train_backend("hip")).  fp32, NCHW.
//
// No index map and no selector are stored by the forward: the backward rescans y, the pool's input, with the forward's own
// rule (tpspp_crnn.hip: row by row, `v > m || v != v` replaces m), as the fused BatchNorm + pool kernels of
// tpspp_bn_pool_train.hip rescan z.  A window's selected element is the last one that replaced m; a window in which nothing
// did (every element inside the map is -inf) selects its first element inside the map, as ATen's index does.
//
// dy is GATHERED: a lane owns elements of dy and adds dp over the windows that contain the element and selected it, in
// ascending (oh, ow), starting from +0.  No atomics, no workspace; an element no window covers, and with relu_mask = 1 an
// element with !(y > 0), is +0.
//   * maxpool_bwd_kernel: one lane per element of y; it visits the at most ceil(kh / sh) ceil(kw / sw) windows around it
//     and rescans each (K22: the 2x2 window as compile-time trip counts -- every pool of the VGG).
//   * maxpool2x2_bwd_vec_kernel: kernel 2x2, stride 2, no padding, W % 4 == 0, 16-byte aligned y and dy, 8-byte aligned dp.
//     Windows do not overlap, so a lane owns two windows side by side, both rows: one 16-byte load of y per row, dp's
//     8 bytes, one 16-byte store per row (bn_pool_bwd_data_kernel<true>'s shape).  The last row of an odd H is +0.
//
// Replaces (reference, mmocr/models/textrecog/): the autograd of nn.MaxPool2d and of the nn.ReLU(True) in front of it,
// backbones/very_deep_vgg.py:39-60.
#include "tpspp_common.h"

namespace {

constexpr int kThreads = 256;

struct PoolGeo {
    unsigned H, W, Ho, Wo;
    int kh, kw, sh, sw, ph, pw;
};

// Is (h, w) the selected element of window (oh, ow)?  The scan of the forward on the same bits.
template <bool K22>
__device__ __forceinline__ bool selects(const float* __restrict__ plane, const PoolGeo& g, int oh, int ow, int h, int w)
{
    const int kh = K22 ? 2 : g.kh, kw = K22 ? 2 : g.kw;
    const int y0 = oh * g.sh - g.ph, x0 = ow * g.sw - g.pw;
    float m = -INFINITY;
    int sy = y0 < 0 ? 0 : y0, sx = x0 < 0 ? 0 : x0;     // nothing replaced m: the first element inside the map
#pragma unroll
    for (int i = 0; i < kh; ++i) {
        const int y = y0 + i;
        if (y < 0 || y >= (int)g.H) continue;
#pragma unroll
        for (int j = 0; j < kw; ++j) {
            const int x = x0 + j;
            if (x < 0 || x >= (int)g.W) continue;
            const float v = plane[(unsigned)y * g.W + (unsigned)x];
            if (v > m || v != v) {
                m = v;
                sy = y;
                sx = x;
            }
        }
    }
    return sy == h && sx == w;
}

__device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

template <bool K22>
__global__ void __launch_bounds__(kThreads)
maxpool_bwd_kernel(const float* __restrict__ dp, const float* __restrict__ y, int relu_mask, PoolGeo g, unsigned total,
                   float* __restrict__ dy)
{
    const unsigned e = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (e >= total) return;
    const int w = (int)(e % g.W);
    const unsigned t = e / g.W;
    const int h = (int)(t % g.H);
    const unsigned pl = t / g.H;
    const int kh = K22 ? 2 : g.kh, kw = K22 ? 2 : g.kw;
    // windows that contain (h, w): oh sh - ph <= h <= oh sh - ph + kh - 1
    int oh0 = floor_div(h + g.ph - kh + g.sh, g.sh), oh1 = (h + g.ph) / g.sh;
    int ow0 = floor_div(w + g.pw - kw + g.sw, g.sw), ow1 = (w + g.pw) / g.sw;
    oh0 = oh0 < 0 ? 0 : oh0;
    ow0 = ow0 < 0 ? 0 : ow0;
    oh1 = oh1 > (int)g.Ho - 1 ? (int)g.Ho - 1 : oh1;
    ow1 = ow1 > (int)g.Wo - 1 ? (int)g.Wo - 1 : ow1;
    const float* plane = y + (size_t)pl * g.H * g.W;
    const float* gp = dp + (size_t)pl * g.Ho * g.Wo;
    float acc = 0.0f;
    if (!relu_mask || y[e] > 0.0f) {
        for (int oh = oh0; oh <= oh1; ++oh)
            for (int ow = ow0; ow <= ow1; ++ow)
                if (selects<K22>(plane, g, oh, ow, h, w)) acc = acc + gp[(unsigned)oh * g.Wo + (unsigned)ow];
    }
    dy[e] = acc;
}

// the 2x2 scan of one window without padding -> the selected index 0..3 (row-major)
__device__ __forceinline__ int scan4(float a00, float a01, float a10, float a11)
{
    float m = -INFINITY;
    int k = 0;
    if (a00 > m || a00 != a00) { m = a00; k = 0; }
    if (a01 > m || a01 != a01) { m = a01; k = 1; }
    if (a10 > m || a10 != a10) { m = a10; k = 2; }
    if (a11 > m || a11 != a11) { m = a11; k = 3; }
    return k;
}

__device__ __forceinline__ float pick(bool sel, float v, float gr, int relu_mask)
{
    return sel && (!relu_mask || v > 0.0f) ? 0.0f + gr : 0.0f;
}

// unit = two 2x2 cells side by side of the ceil(H/2) x (W/4) grid: (pl, cy, cxu)
__global__ void __launch_bounds__(kThreads)
maxpool2x2_bwd_vec_kernel(const float* __restrict__ dp, const float* __restrict__ y, int relu_mask, unsigned H, unsigned W,
                          unsigned Ho, unsigned Wo, unsigned Hc, unsigned Wu, unsigned units, float* __restrict__ dy)
{
    const unsigned u = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (u >= units) return;
    const unsigned cxu = u % Wu;
    const unsigned t = u / Wu;
    const unsigned cy = t % Hc;
    const unsigned pl = t / Hc;
    const size_t e0 = ((size_t)pl * H + 2u * cy) * W + 4u * cxu;
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (2u * cy + 1u < H) {
        const size_t e1 = e0 + W;
        const float4 a = *reinterpret_cast<const float4*>(y + e0);
        const float4 b = *reinterpret_cast<const float4*>(y + e1);
        const float2 gr = *reinterpret_cast<const float2*>(dp + ((size_t)pl * Ho + cy) * Wo + 2u * cxu);
        const int k0 = scan4(a.x, a.y, b.x, b.y), k1 = scan4(a.z, a.w, b.z, b.w);
        float4 o1;
        o0.x = pick(k0 == 0, a.x, gr.x, relu_mask);
        o0.y = pick(k0 == 1, a.y, gr.x, relu_mask);
        o1.x = pick(k0 == 2, b.x, gr.x, relu_mask);
        o1.y = pick(k0 == 3, b.y, gr.x, relu_mask);
        o0.z = pick(k1 == 0, a.z, gr.y, relu_mask);
        o0.w = pick(k1 == 1, a.w, gr.y, relu_mask);
        o1.z = pick(k1 == 2, b.z, gr.y, relu_mask);
        o1.w = pick(k1 == 3, b.w, gr.y, relu_mask);
        *reinterpret_cast<float4*>(dy + e1) = o1;
    }
    *reinterpret_cast<float4*>(dy + e0) = o0;
}

inline bool aligned(const void* p, uintptr_t bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

}  // namespace

TPSPP_EXPORT int tpspp_crnn_maxpool_bwd(const float* dp, const float* y, int relu_mask, int N, int C, int H, int W, int kh,
                                        int kw, int sh, int sw, int ph, int pw, float* dy, int Ho, int Wo,
                                        tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_maxpool_bwd";
    TPSPP_REQUIRE(dp && y && dy, "%s: null pointer", who);
    TPSPP_REQUIRE(relu_mask == 0 || relu_mask == 1, "%s: relu_mask must be 0 or 1", who);
    TPSPP_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1, "%s: kernel and stride must be >= 1", who);
    TPSPP_REQUIRE(ph >= 0 && pw >= 0 && ph <= kh / 2 && pw <= kw / 2, "%s: padding must be 0 .. half the kernel size", who);
    TPSPP_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: the padded map is smaller than the kernel", who);
    const int ho = (H + 2 * ph - kh) / sh + 1, wo = (W + 2 * pw - kw) / sw + 1;
    TPSPP_REQUIRE(Ho == ho && Wo == wo, "%s: Ho x Wo must be %d x %d, got %d x %d", who, ho, wo, Ho, Wo);
    const long long total = (long long)N * C * H * W;
    TPSPP_REQUIRE(total <= 0x7fffffffLL && (long long)N * C * Ho * Wo <= 0x7fffffffLL, "%s: more than 2^31 - 1 elements", who);
    if (N == 0) return TPSPP_OK;
    hipStream_t st = tpspp::as_stream(stream);
    const bool k22 = kh == 2 && kw == 2;
    if (k22 && sh == 2 && sw == 2 && ph == 0 && pw == 0 && W % 4 == 0 && aligned(y, 16) && aligned(dy, 16) && aligned(dp, 8)) {
        const unsigned Hc = ((unsigned)H + 1) / 2, Wu = (unsigned)W / 4;
        const unsigned units = (unsigned)N * C * Hc * Wu;
        hipLaunchKernelGGL(maxpool2x2_bwd_vec_kernel, dim3((units + kThreads - 1) / kThreads), dim3(kThreads), 0, st, dp, y,
                           relu_mask, (unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, Hc, Wu, units, dy);
        return tpspp::check_launch(who);
    }
    const PoolGeo g{(unsigned)H, (unsigned)W, (unsigned)Ho, (unsigned)Wo, kh, kw, sh, sw, ph, pw};
    const dim3 grid(((unsigned)total + kThreads - 1) / kThreads);
    if (k22)
        hipLaunchKernelGGL(maxpool_bwd_kernel<true>, grid, dim3(kThreads), 0, st, dp, y, relu_mask, g, (unsigned)total, dy);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<false>, grid, dim3(kThreads), 0, st, dp, y, relu_mask, g, (unsigned)total, dy);
    return tpspp::check_launch(who);
}
