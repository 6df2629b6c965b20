// The CRNN recogniser's kernels (include/crnn/tpspp_crnn.h): rectangular max-pooling, the recurrence of a bidirectional
// LSTM layer and the CTC greedy decode.
// Replaces: nn.MaxPool2d in backbones/very_deep_vgg.py:51-60, nn.LSTM's recurrence in layers/lstm_layer.py:10,14 and
// F.softmax + topk(1) + the collapse scan of convertors/ctc.py:110-137 (reference).
#include <climits>

#include "crnn/tpspp_crnn.h"
#include "tpspp_common.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;

typedef float f32x4 __attribute__((ext_vector_type(4)));

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
constexpr int kHid = TPSPP_CRNN_HIDDEN;     // units per direction
constexpr int kGates = 4 * kHid;            // gate columns per direction: i, f, g, o
constexpr int kRows = 16;                   // image rows of the matrix-core tile
constexpr int kLd = kHid + 4;               // LDS row stride of h in floats: 16-byte aligned, rows 4 banks apart
constexpr int kLstmThreads = 512;           // 8 wavefronts, each owns 2 tiles of 16 units with their 4 gates

__device__ __forceinline__ float sigmoid_safe(float x)
{
    const float e = expf(-fabsf(x));        // (0, 1]
    return (x >= 0.0f ? 1.0f : e) / (1.0f + e);
}

__device__ __forceinline__ float tanh_safe(float x)
{
    const float m = expm1f(-2.0f * fabsf(x));   // (-1, 0]
    return copysignf(-m / (m + 2.0f), x);
}

// blockIdx.x = 2 * block-of-images + direction.  Lane l of a wavefront holds, as the A operand, h[image l & 15][k] and, as
// the B operand, w_hh[unit l & 15][k] for k = 16 b + 4 (l >> 4) + m; its accumulators hold images 4 (l >> 4) + r of unit
// l & 15 -- the same (image, unit) in all four gate tiles, so the cell update needs no exchange and c stays in registers.
__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_kernel(const float* __restrict__ xg, const float* __restrict__ whh, float* __restrict__ out, int T, int N, int g)
{
    __shared__ __attribute__((aligned(16))) float hbuf[2][kRows * kLd];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int d = blockIdx.x & 1;
    const int n0 = (int)(blockIdx.x >> 1) * g;
    const int col = lane & 15, quad = lane >> 4;
    for (int i = tid; i < 2 * kRows * kLd; i += kLstmThreads) (&hbuf[0][0])[i] = 0.0f;
    const float* w = whh + (size_t)d * kGates * kHid;
    float c[2][4];
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        c[0][r] = c[1][r] = 0.0f;
        valid[r] = 4 * quad + r < g && n0 + 4 * quad + r < N;
    }
    int cur = 0;
    __syncthreads();
    for (int s = 0; s < T; ++s) {
        const int t = d ? T - 1 - s : s;
        const float* hrow = &hbuf[cur][col * kLd + 4 * quad];
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int u = (2 * wave + ut) * 16 + col;
            f32x4 acc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* x = xg + (((size_t)t * N + (valid[r] ? n0 + 4 * quad + r : 0)) * 2 + d) * kGates + u;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q][r] = valid[r] ? x[q * kHid] : 0.0f;
            }
            const float* wr = w + (size_t)u * kHid + 4 * quad;
            // (h is read from LDS again per tile: 16 rows of A held in registers next to the weight loads in flight spill)
#pragma unroll 4
            for (int b = 0; b < 16; ++b) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(hrow + 16 * b);
                f32x4 bv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) bv[q] = *reinterpret_cast<const f32x4*>(wr + (size_t)q * kHid * kHid + 16 * b);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv[q][m], acc[q], 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gi = sigmoid_safe(acc[0][r]), gf = sigmoid_safe(acc[1][r]);
                const float gg = tanh_safe(acc[2][r]), go = sigmoid_safe(acc[3][r]);
                c[ut][r] = gf * c[ut][r] + gi * gg;
                const float h = go * tanh_safe(c[ut][r]);
                hbuf[cur ^ 1][(4 * quad + r) * kLd + u] = h;        // rows past the block: xg = 0 keeps c = h = 0
                if (valid[r]) out[((size_t)t * N + n0 + 4 * quad + r) * (2 * kHid) + d * kHid + u] = h;
            }
        }
        __syncthreads();            // h of this step is complete before any wavefront reads it; the other copy is free
        cur ^= 1;
    }
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

bool lstm_group_ok(int g) { return g == 4 || g == 8 || g == 16; }

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
    TPSPP_REQUIRE(hidden == kHid, "%s: hidden must be %d, got %d", who, kHid, hidden);
    TPSPP_REQUIRE(T >= 1 && N >= 0, "%s: bad sizes (T >= 1, N >= 0)", who);
    TPSPP_REQUIRE(images_per_group == 0 || lstm_group_ok(images_per_group), "%s: images_per_group must be 0, 4, 8 or 16, got %d",
                  who, images_per_group);
    TPSPP_REQUIRE((long long)T * N <= (1LL << 30), "%s: T * N too large", who);
    if (N == 0) return TPSPP_OK;
    const int g = tpspp_crnn_lstm_plan(N, images_per_group, 0);
    if (g < 0) return g;
    const unsigned groups = 2u * (unsigned)((N + g - 1) / g);
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
