// Max-pooling on the blocked feature maps the bf16 convolutions exchange (include/tpspp_crnn_bf16.h): (N, C/8, H, W, 8)
// in bf16 (layout code 2) or fp32 (code 3), so that VeryDeepVgg's maps stay blocked between its convolutions in the reduced
// modes.  Memory-bound: one thread per (image, channel group, output pixel), a window position is one 16-byte load (bf16) or
// two (fp32), the result as many 16-byte stores; consecutive lanes take consecutive output columns, i.e. consecutive
// 16- / 32-byte units of a row.  No LDS, no atomics; the eight running maxima live in registers.
// Replaces: nn.MaxPool2d in backbones/very_deep_vgg.py:51-60 (reference) when the module runs in bf16 / bf16x3.
#include "tpspp_crnn_bf16.h"
#include "tpspp_common.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;

// ATen's rule: a NaN is taken, and stays
__device__ __forceinline__ float pool_take(float m, float v) { return (v > m || v != v) ? v : m; }

template <bool F32>
__global__ void __launch_bounds__(256)
crnn_maxpool_blk_kernel(const u32x4* __restrict__ in, u32x4* __restrict__ out, long long total, int H, int W, int kh, int kw,
                        int sh, int sw, int ph, int pw, int Ho, int Wo)
{
    constexpr int U = F32 ? 2 : 1;                      // 16-byte units per (pixel, channel group)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo);
    const long long t = i / Wo;
    const int oy = (int)(t % Ho);
    const u32x4* plane = in + (t / Ho) * ((long long)H * W * U);        // (image, channel group)
    const int y0 = oy * sh - ph, x0 = ox * sw - pw;
    float m[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) m[c] = -INFINITY;
    for (int dy = 0; dy < kh; ++dy) {
        const int y = y0 + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = 0; dx < kw; ++dx) {
            const int x = x0 + dx;
            if (x < 0 || x >= W) continue;
            const u32x4* p = plane + ((long long)y * W + x) * U;
            if constexpr (F32) {
                const u32x4 a = p[0], b = p[1];
#pragma unroll
                for (int c = 0; c < 4; ++c) {           // (by value: a bit cast of the vector element itself reads element 0)
                    const unsigned ua = a[c], ub = b[c];
                    m[c] = pool_take(m[c], __builtin_bit_cast(float, ua));
                    m[4 + c] = pool_take(m[4 + c], __builtin_bit_cast(float, ub));
                }
            } else {
                const u32x4 a = p[0];
#pragma unroll
                for (int c = 0; c < 4; ++c) {           // widening a bf16 is exact: the maximum is one of the inputs
                    m[2 * c] = pool_take(m[2 * c], __builtin_bit_cast(float, a[c] << 16));
                    m[2 * c + 1] = pool_take(m[2 * c + 1], __builtin_bit_cast(float, a[c] & 0xffff0000u));
                }
            }
        }
    }
    u32x4* o = out + i * U;
    if constexpr (F32) {
        u32x4 a, b;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = __builtin_bit_cast(unsigned, m[c]);
            b[c] = __builtin_bit_cast(unsigned, m[4 + c]);
        }
        o[0] = a;
        o[1] = b;
    } else {
        u32x4 a;
#pragma unroll
        for (int c = 0; c < 4; ++c)                      // (the low 16 bits of a widened bf16 are zero)
            a[c] = (__builtin_bit_cast(unsigned, m[2 * c]) >> 16) | (__builtin_bit_cast(unsigned, m[2 * c + 1]) & 0xffff0000u);
        o[0] = a;
    }
}

}  // namespace

TPSPP_EXPORT int tpspp_crnn_maxpool_blk_fwd(const void* in, int layout, int N, int C, int H, int W, int kh, int kw, int sh,
                                            int sw, int ph, int pw, void* out, int Ho, int Wo, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_maxpool_blk_fwd";
    TPSPP_REQUIRE(in && out, "%s: null pointer", who);
    TPSPP_REQUIRE(layout == 2 || layout == 3, "%s: layout must be 2 (bf16 blocked) or 3 (fp32 blocked), got %d", who, layout);
    TPSPP_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(C % 8 == 0, "%s: a blocked map needs a multiple of 8 channels, got %d", who, C);
    TPSPP_REQUIRE(((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & 15) == 0, "%s: pointers must be 16-byte aligned",
                  who);
    TPSPP_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1, "%s: kernel and stride must be >= 1", who);
    TPSPP_REQUIRE(ph >= 0 && pw >= 0 && ph <= kh / 2 && pw <= kw / 2, "%s: padding must be 0 .. half the kernel size", who);
    TPSPP_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: the padded map is smaller than the kernel", who);
    const int ho = (H + 2 * ph - kh) / sh + 1, wo = (W + 2 * pw - kw) / sw + 1;
    TPSPP_REQUIRE(Ho == ho && Wo == wo, "%s: Ho x Wo must be %d x %d, got %d x %d", who, ho, wo, Ho, Wo);
    const long long total = (long long)N * (C / 8) * Ho * Wo;
    if (total == 0) return TPSPP_OK;
    TPSPP_REQUIRE((total + 255) / 256 < (1LL << 31), "%s: too large", who);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const u32x4* src = reinterpret_cast<const u32x4*>(in);
    u32x4* dst = reinterpret_cast<u32x4*>(out);
    if (layout == 3)
        hipLaunchKernelGGL(crnn_maxpool_blk_kernel<true>, grid, block, 0, tpspp::as_stream(stream), src, dst, total, H, W, kh, kw,
                           sh, sw, ph, pw, Ho, Wo);
    else
        hipLaunchKernelGGL(crnn_maxpool_blk_kernel<false>, grid, block, 0, tpspp::as_stream(stream), src, dst, total, H, W, kh, kw,
                           sh, sw, ph, pw, Ho, Wo);
    return tpspp::check_launch(who);
}
