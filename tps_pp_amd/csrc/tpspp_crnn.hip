// The CRNN recogniser's kernels (include/tpspp_crnn.h): rectangular max-pooling, the recurrence of a bidirectional
// LSTM layer and the CTC greedy decode.
// Replaces: nn.MaxPool2d in backbones/very_deep_vgg.py:51-60, nn.LSTM's recurrence in layers/lstm_layer.py:10,14 and
// F.softmax + topk(1) + the collapse scan of convertors/ctc.py:110-137 (reference).
#include <climits>

#include "tpspp_crnn.h"
#include "tpspp_common.h"
#include "tpspp_crnn_cell.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;
using namespace tpspp_crnn_cell;

// ---- max-pooling -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
crnn_maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, long long total, int H, int W, int kh, int kw,
                    int sh, int sw, int ph, int pw, int Ho, int Wo)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo);
    const long long t = i / Wo;
    const int oy = (int)(t % Ho);
    const float* plane = in + (t / Ho) * (long long)H * W;
    const int y0 = oy * sh - ph, x0 = ox * sw - pw;
    float m = -INFINITY;
    for (int dy = 0; dy < kh; ++dy) {
        const int y = y0 + dy;
        if (y < 0 || y >= H) continue;
        for (int dx = 0; dx < kw; ++dx) {
            const int x = x0 + dx;
            if (x < 0 || x >= W) continue;
            const float v = plane[(long long)y * W + x];
            m = (v > m || v != v) ? v : m;              // ATen's rule: a NaN is taken, and stays
        }
    }
    out[i] = m;
}

// ---- the LSTM recurrence -----------------------------------------------------------------------------------------------------
// (the body, its fp32 product and the entry points' shared checks: tpspp_crnn_cell.h)
__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_kernel(const float* __restrict__ xg, const float* __restrict__ whh, float* __restrict__ out, int T, int N, int g)
{
    lstm_forward<MulF32, false>(xg, whh, out, nullptr, nullptr, T, N, g);
}

// ---- CTC greedy decode -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
crnn_ctc_decode_kernel(const float* __restrict__ logits, const int* __restrict__ decode_len, int N, int T, int C, int blank,
                       int* __restrict__ idx, float* __restrict__ score)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const int len = decode_len[n];
    int prev = blank;
    for (int t = 0; t < T; ++t) {
        const float* row = logits + ((size_t)n * T + t) * C;
        float mx = -INFINITY;
        int am = INT_MAX;
        for (int k = lane; k < C; k += kWave) {
            const float v = row[k];
            if (am == INT_MAX || v > mx) { mx = v; am = k; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(mx, off, kWave);
            const int oi = __shfl_xor(am, off, kWave);
            if (oi != INT_MAX && (am == INT_MAX || ov > mx || (ov == mx && oi < am))) { mx = ov; am = oi; }
        }
        float sum = 0.0f;
        for (int k = lane; k < C; k += kWave) sum += expf(row[k] - mx);
        sum = wave_sum(sum);
        const bool keep = t < len && am != blank && am != prev;
        if (lane == 0) {
            idx[(size_t)n * T + t] = keep ? am : -1;
            score[(size_t)n * T + t] = keep ? 1.0f / sum : 0.0f;
        }
        prev = am;
    }
}

int lstm_plan(int N, int images_per_group, int cus)
{
    if (images_per_group != 0) return images_per_group;
    for (int g = 16; g > 4; g >>= 1)
        if (2LL * ((N + g - 1) / g) >= cus) return g;
    return 4;
}

}  // namespace

TPSPP_EXPORT int tpspp_crnn_maxpool_fwd(const float* in, int N, int C, int H, int W, int kh, int kw, int sh, int sw, int ph,
                                        int pw, float* out, int Ho, int Wo, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_maxpool_fwd";
    TPSPP_REQUIRE(in && out, "%s: null pointer", who);
    TPSPP_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1, "%s: kernel and stride must be >= 1", who);
    TPSPP_REQUIRE(ph >= 0 && pw >= 0 && ph <= kh / 2 && pw <= kw / 2, "%s: padding must be 0 .. half the kernel size", who);
    TPSPP_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: the padded map is smaller than the kernel", who);
    const int ho = (H + 2 * ph - kh) / sh + 1, wo = (W + 2 * pw - kw) / sw + 1;
    TPSPP_REQUIRE(Ho == ho && Wo == wo, "%s: Ho x Wo must be %d x %d, got %d x %d", who, ho, wo, Ho, Wo);
    const long long total = (long long)N * C * Ho * Wo;
    if (total == 0) return TPSPP_OK;
    TPSPP_REQUIRE((total + 255) / 256 < (1LL << 31), "%s: too large", who);
    hipLaunchKernelGGL(crnn_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tpspp::as_stream(stream), in,
                       out, total, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_crnn_lstm_plan(int N, int images_per_group, int compute_units)
{
    const char* who = "tpspp_crnn_lstm_plan";
    TPSPP_REQUIRE(N >= 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(images_per_group == 0 || lstm_group_ok(images_per_group), "%s: images_per_group must be 0, 4, 8 or 16, got %d",
                  who, images_per_group);
    if (compute_units <= 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        compute_units = 256;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            compute_units = prop.multiProcessorCount;
        (void)hipGetLastError();            // no device: not this call's error
    }
    return lstm_plan(N, images_per_group, compute_units);
}

TPSPP_EXPORT int tpspp_crnn_lstm_fwd(const float* xg, const float* w_hh, float* out, int T, int N, int hidden,
                                     int images_per_group, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_fwd";
    TPSPP_REQUIRE(xg && w_hh && out, "%s: null pointer", who);
    const int rc = check_lstm(who, T, N, hidden, images_per_group);
    if (rc != TPSPP_OK || N == 0) return rc;
    unsigned groups;
    const int g = lstm_grid(N, images_per_group, groups);
    if (g < 0) return g;
    hipLaunchKernelGGL(crnn_lstm_kernel, dim3(groups), dim3(kLstmThreads), 0, tpspp::as_stream(stream), xg, w_hh, out, T, N, g);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_crnn_ctc_decode(const float* logits, const int* decode_len, int N, int T, int C, int blank, int* idx,
                                       float* score, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_ctc_decode";
    TPSPP_REQUIRE(logits && decode_len && idx && score, "%s: null pointer", who);
    TPSPP_REQUIRE(N >= 0 && T >= 1, "%s: bad sizes (N >= 0, T >= 1)", who);
    TPSPP_REQUIRE(C >= 2, "%s: C must be >= 2, got %d", who, C);
    TPSPP_REQUIRE(blank >= 0 && blank < C, "%s: blank %d out of range 0 .. %d", who, blank, C - 1);
    TPSPP_REQUIRE((long long)N * T <= (1LL << 30), "%s: N * T too large", who);
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(crnn_ctc_decode_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, tpspp::as_stream(stream), logits,
                       decode_len, N, T, C, blank, idx, score);
    return tpspp::check_launch(who);
}
