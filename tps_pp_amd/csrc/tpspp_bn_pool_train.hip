// BatchNorm + ReLU + MaxPool2d(2, 2) as one pass, forward and backward, and the backward of AdaptiveAvgPool2d(1): the new
// kernels of the classic rectifier's localisation network in training (TPSPreprocessor.set_train_backend("hip")).
// fp32, NCHW, statistics per channel over M = N*H*W as in tpspp_bn_train.hip.
//
//   a(v) = relu((v - mean_c) * (gamma_c rstd_c) + beta_c)      (tpspp_bn_pool.h: bn_apply_kernel's expression)
//
//   * bn_pool_fwd_kernel: p = the 2x2 / stride 2 max-pool of a(z), scanned with ATen's rule.  The activated
//     full-resolution map is never written, and no selector is: both backward kernels stream z anyway (xhat needs it) and
//     find the selected element again with the same scan on the same bits.
//   * bn_pool_bwd_reduce_kernel + bn_pool_bwd_combine_kernel: dr is dp at a window's selected element where a(.) > 0 and
//     +0 everywhere else; per channel sum dr and sum dr xhat (the beta and gamma gradients).  Only windows carry a
//     non-zero dr, so the kernel walks windows.  FIXED SPLIT: S = ceil(M / 4096) slices of 1024 windows each (a channel
//     has at most M / 4 windows), partials to the caller's workspace, slices added in slice order in fp64.
//   * bn_pool_bwd_data_kernel: dz = gamma rstd (dr - sum dr / M - xhat sum dr xhat / M) (batch statistics) or
//     gamma rstd dr (running statistics) for every element of z, the row and column no window covers included.
//   * global_avgpool_bwd_kernel: dx[n][c][:][:] = g[n][c] / (H W).
// A lane owns whole windows (both rows), so nothing is exchanged.  The float4 forms hold one row pair of two windows per
// lane and need W % 4 == 0 (every row then starts on 16 bytes); anything else, the 8x25 map of the third layer included,
// takes the scalar forms, one window per lane.  No atomics, no allocation, no host synchronisation.
//
// Replaces (reference, mmocr/models/textrecog/): nn.BatchNorm2d + nn.ReLU + nn.MaxPool2d(2, 2) and nn.AdaptiveAvgPool2d(1)
// of preprocessor/tps_preprocessor.py:101-128, forward and autograd.
#include "tpspp_common.h"
#include "tpspp_bn_pool.h"
#include "tpspp_dev.h"

#include <initializer_list>

namespace {

using tpspp_bn_pool::Act;
using tpspp_bn_pool::bn_relu;
using tpspp_bn_pool::load_act;
using tpspp_bn_pool::scan2x2;
using tpspp_dev::block_sums;

constexpr int kThreads = 256;
constexpr int kSlice = 4096;                      // full-resolution elements of a channel per slice
constexpr int kSliceWin = kSlice / 4;             // windows of a channel per slice
constexpr int kCombine = 64;

inline long long pool_slices(long long M) { return (M + kSlice - 1) / kSlice; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }

// ------------------------------------------------------------------------------------------------------------------
// forward.  Scalar: unit = one window (pl, oy, ox).  VEC: unit = two windows side by side (pl, oy, 2 oxp .. 2 oxp + 1).
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_pool_fwd_kernel(const float* __restrict__ z, const float* __restrict__ mean, const float* __restrict__ rstd,
                   const float* __restrict__ gamma, const float* __restrict__ beta, unsigned C, unsigned H, unsigned W,
                   unsigned Ho, unsigned Wo, unsigned units, float* __restrict__ p)
{
    const unsigned u = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (u >= units) return;
    const unsigned Wu = VEC ? Wo / 2 : Wo;
    const unsigned oxu = u % Wu;
    const unsigned t = u / Wu;
    const unsigned oy = t % Ho;
    const unsigned pl = t / Ho;
    const Act k = load_act(mean, rstd, gamma, beta, pl % C);
    const float* r0 = z + ((size_t)pl * H + 2u * oy) * W + (VEC ? 4u : 2u) * oxu;
    const float* r1 = r0 + W;
    float m;
    if (VEC) {
        const float4 a = ld4(r0), b = ld4(r1);
        float2 o;
        scan2x2(bn_relu(a.x, k), bn_relu(a.y, k), bn_relu(b.x, k), bn_relu(b.y, k), m);
        o.x = m;
        scan2x2(bn_relu(a.z, k), bn_relu(a.w, k), bn_relu(b.z, k), bn_relu(b.w, k), m);
        o.y = m;
        *reinterpret_cast<float2*>(p + (size_t)u * 2) = o;
    } else {
        scan2x2(bn_relu(r0[0], k), bn_relu(r0[1], k), bn_relu(r1[0], k), bn_relu(r1[1], k), m);
        p[u] = m;
    }
}

// dr and xhat of a window's selected element: acc += (dr, dr xhat)
__device__ __forceinline__ void window_sums(float z00, float z01, float z10, float z11, float g, const Act& k, float rs,
                                            float (&acc)[2])
{
    float m;
    const int sel = scan2x2(bn_relu(z00, k), bn_relu(z01, k), bn_relu(z10, k), bn_relu(z11, k), m);
    const float zs = sel == 0 ? z00 : sel == 1 ? z01 : sel == 2 ? z10 : z11;
    const float dr = m > 0.0f ? g : 0.0f;
    acc[0] = acc[0] + dr;
    acc[1] = acc[1] + dr * ((zs - k.mean) * rs);
}

// ------------------------------------------------------------------------------------------------------------------
// backward reduction: slice s of channel c -> ws[(s * C + c) * 2 + {0, 1}] = (sum dr, sum dr xhat) over the windows
// s * 1024 .. s * 1024 + 1023 of the channel (windows numbered (n, oy, ox)); a slice past the last window writes zeros
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_pool_bwd_reduce_kernel(const float* __restrict__ dp, const float* __restrict__ z, const float* __restrict__ mean,
                          const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                          unsigned C, unsigned H, unsigned W, unsigned Ho, unsigned Wo, unsigned units,
                          float* __restrict__ ws)
{
    __shared__ float red[2][4];
    constexpr int PER = VEC ? 2 : 1;              // windows per unit
    const unsigned s = blockIdx.x, c = blockIdx.y;
    const Act k = load_act(mean, rstd, gamma, beta, c);
    const float rs = rstd[c];
    const unsigned Wu = VEC ? Wo / 2 : Wo;
    float acc[2] = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < kSliceWin / PER / kThreads; ++j) {
        const unsigned u = s * (unsigned)(kSliceWin / PER) + (unsigned)(j * kThreads) + threadIdx.x;
        if (u >= units) continue;
        const unsigned oxu = u % Wu;
        const unsigned t = u / Wu;
        const unsigned oy = t % Ho;
        const unsigned pl = (t / Ho) * C + c;
        const float* r0 = z + ((size_t)pl * H + 2u * oy) * W + (VEC ? 4u : 2u) * oxu;
        const float* r1 = r0 + W;
        const float* gp = dp + ((size_t)pl * Ho + oy) * Wo + (VEC ? 2u : 1u) * oxu;
        if (VEC) {
            const float4 a = ld4(r0), b = ld4(r1);
            const float2 g = ld2(gp);
            window_sums(a.x, a.y, b.x, b.y, g.x, k, rs, acc);
            window_sums(a.z, a.w, b.z, b.w, g.y, k, rs, acc);
        } else {
            window_sums(r0[0], r0[1], r1[0], r1[1], gp[0], k, rs, acc);
        }
    }
    block_sums<2>(acc, red);
    if (threadIdx.x == 0) {
        float* w = ws + ((size_t)s * C + c) * 2;
        w[0] = acc[0];
        w[1] = acc[1];
    }
}

// one thread per channel: the slices in slice order, fp64
__global__ void __launch_bounds__(kCombine)
bn_pool_bwd_combine_kernel(const float* __restrict__ ws, int S, int C, float* __restrict__ s_dr, float* __restrict__ s_x)
{
    const int c = blockIdx.x * kCombine + threadIdx.x;
    if (c >= C) return;
    double t0 = 0.0, t1 = 0.0;
    for (int s = 0; s < S; ++s) {
        const float2 w = ld2(ws + ((size_t)s * C + c) * 2);
        t0 = t0 + (double)w.x;
        t1 = t1 + (double)w.y;
    }
    s_dr[c] = (float)t0;
    s_x[c] = (float)t1;
}

// ------------------------------------------------------------------------------------------------------------------
// per-channel constants of the data gradient
struct Grad {
    float mean, rs, sc, k0, k1;
    int train;
};

// dz of one element (bn_bwd_data_kernel's expression); + 0 turns the -0 of a negative gamma times +0 into +0
__device__ __forceinline__ float dz_of(float dr, float zv, const Grad& q)
{
    if (q.train) return q.sc * ((dr - q.k0) - ((zv - q.mean) * q.rs) * q.k1) + 0.0f;
    return q.sc * dr + 0.0f;
}

// dz of a window's four elements from its upstream gradient g
__device__ __forceinline__ void window_dz(float z00, float z01, float z10, float z11, float g, const Act& k, const Grad& q,
                                          float (&o)[4])
{
    float m;
    const int sel = scan2x2(bn_relu(z00, k), bn_relu(z01, k), bn_relu(z10, k), bn_relu(z11, k), m);
    const float dr = m > 0.0f ? g : 0.0f;
    o[0] = dz_of(sel == 0 ? dr : 0.0f, z00, q);
    o[1] = dz_of(sel == 1 ? dr : 0.0f, z01, q);
    o[2] = dz_of(sel == 2 ? dr : 0.0f, z10, q);
    o[3] = dz_of(sel == 3 ? dr : 0.0f, z11, q);
}

// Scalar: unit = one cell (pl, cy, cx) of the ceil(H/2) x ceil(W/2) grid of 2x2 cells; a cell that lacks its second row or
// column is no window: its elements have dr = +0.  VEC (W % 4 == 0): unit = two cells side by side, the second row absent
// in the last cell row of an odd H.
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_pool_bwd_data_kernel(const float* __restrict__ dp, const float* __restrict__ z, const float* __restrict__ mean,
                        const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                        const float* __restrict__ s_dr, const float* __restrict__ s_x, int train, float inv_m, unsigned C,
                        unsigned H, unsigned W, unsigned Ho, unsigned Wo, unsigned Hc, unsigned Wu, unsigned units,
                        float* __restrict__ dz)
{
    const unsigned u = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if (u >= units) return;
    const unsigned cxu = u % Wu;
    const unsigned t = u / Wu;
    const unsigned cy = t % Hc;
    const unsigned pl = t / Hc;
    const unsigned c = pl % C;
    const Act k = load_act(mean, rstd, gamma, beta, c);
    Grad q;
    q.mean = k.mean;
    q.rs = rstd[c];
    q.sc = k.scale;
    q.train = train;
    q.k0 = train ? s_dr[c] * inv_m : 0.0f;
    q.k1 = train ? s_x[c] * inv_m : 0.0f;
    const bool row1 = 2u * cy + 1u < H;
    const size_t e0 = ((size_t)pl * H + 2u * cy) * W + (VEC ? 4u : 2u) * cxu;
    const size_t e1 = e0 + W;
    float* d0 = dz + e0;
    float* d1 = dz + e1;
    if (VEC) {
        const float4 a = ld4(z + e0);
        float4 o0, o1;
        if (row1) {
            const float4 b = ld4(z + e1);
            const float2 g = ld2(dp + ((size_t)pl * Ho + cy) * Wo + 2u * cxu);
            float o[4];
            window_dz(a.x, a.y, b.x, b.y, g.x, k, q, o);
            o0.x = o[0]; o0.y = o[1]; o1.x = o[2]; o1.y = o[3];
            window_dz(a.z, a.w, b.z, b.w, g.y, k, q, o);
            o0.z = o[0]; o0.w = o[1]; o1.z = o[2]; o1.w = o[3];
            *reinterpret_cast<float4*>(d1) = o1;
        } else {
            o0.x = dz_of(0.0f, a.x, q); o0.y = dz_of(0.0f, a.y, q); o0.z = dz_of(0.0f, a.z, q); o0.w = dz_of(0.0f, a.w, q);
        }
        *reinterpret_cast<float4*>(d0) = o0;
    } else {
        const bool col1 = 2u * cxu + 1u < W;
        if (row1 && col1) {
            float o[4];
            window_dz(z[e0], z[e0 + 1], z[e1], z[e1 + 1], dp[((size_t)pl * Ho + cy) * Wo + cxu], k, q, o);
            d0[0] = o[0]; d0[1] = o[1]; d1[0] = o[2]; d1[1] = o[3];
        } else {
            d0[0] = dz_of(0.0f, z[e0], q);
            if (col1) d0[1] = dz_of(0.0f, z[e0 + 1], q);
            if (row1) d1[0] = dz_of(0.0f, z[e1], q);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
global_avgpool_bwd_kernel(const float* __restrict__ g, unsigned HW, unsigned total, float* __restrict__ dx)
{
    constexpr unsigned V = VEC ? 4 : 1;
    const unsigned e = (blockIdx.x * (unsigned)kThreads + threadIdx.x) * V;
    if (e >= total) return;
    const float v = g[e / HW] / (float)HW;        // HW % 4 == 0 in the float4 form: the four elements share a plane
    if (VEC) *reinterpret_cast<float4*>(dx + e) = make_float4(v, v, v, v);
    else dx[e] = v;
}

bool aligned(size_t bytes, std::initializer_list<const void*> ptrs)
{
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % bytes != 0) return false;
    return true;
}

int check_sizes(const char* who, int N, int C, int H, int W)
{
    TPSPP_REQUIRE(N >= 0 && C > 0 && H >= 2 && W >= 2, "%s: bad sizes (N %d, C %d, H %d, W %d; H, W >= 2)", who, N, C, H, W);
    TPSPP_REQUIRE((long long)N * C * H * W <= 0x7fffffffLL, "%s: more than 2^31 - 1 elements", who);
    TPSPP_REQUIRE(C <= 65535, "%s: grid too large (C > 65535)", who);
    return TPSPP_OK;
}

inline dim3 blocks_for(unsigned units) { return dim3((units + kThreads - 1) / kThreads); }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
TPSPP_EXPORT int tpspp_bn_pool2x2_fwd(const float* z, const float* mean, const float* rstd, const float* gamma,
                                      const float* beta, int N, int C, int H, int W, float* p, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_pool2x2_fwd";
    TPSPP_REQUIRE(z && mean && rstd && gamma && beta && p, "%s: null pointer", who);
    int rc = check_sizes(who, N, C, H, W);
    if (rc != TPSPP_OK || N == 0) return rc;
    const unsigned Ho = (unsigned)H / 2, Wo = (unsigned)W / 2;
    const unsigned windows = (unsigned)N * C * Ho * Wo;
    hipStream_t st = tpspp::as_stream(stream);
    if (W % 4 == 0 && aligned(16, {z}) && aligned(8, {p}))
        hipLaunchKernelGGL(bn_pool_fwd_kernel<true>, blocks_for(windows / 2), dim3(kThreads), 0, st, z, mean, rstd, gamma,
                           beta, (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, windows / 2, p);
    else
        hipLaunchKernelGGL(bn_pool_fwd_kernel<false>, blocks_for(windows), dim3(kThreads), 0, st, z, mean, rstd, gamma,
                           beta, (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, windows, p);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_bn_pool2x2_bwd_reduce_workspace_floats(int N, int C, int H, int W)
{
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)pool_slices((long long)N * H * W) * (size_t)C * 2;
}

TPSPP_EXPORT int tpspp_bn_pool2x2_bwd_reduce(const float* dp, const float* z, const float* mean, const float* rstd,
                                             const float* gamma, const float* beta, int N, int C, int H, int W,
                                             float* sum_dr, float* sum_dr_x, float* ws, size_t ws_floats,
                                             tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_pool2x2_bwd_reduce";
    TPSPP_REQUIRE(dp && z && mean && rstd && gamma && beta && sum_dr && sum_dr_x, "%s: null pointer", who);
    int rc = check_sizes(who, N, C, H, W);
    if (rc != TPSPP_OK) return rc;
    const size_t need = tpspp_bn_pool2x2_bwd_reduce_workspace_floats(N, C, H, W);
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_bn_pool2x2_bwd_reduce_workspace_floats(...) = %zu floats, got %zu)", who,
                  need, ws_floats);
    if (N == 0) return TPSPP_OK;
    const unsigned Ho = (unsigned)H / 2, Wo = (unsigned)W / 2;
    const unsigned windows = (unsigned)N * Ho * Wo;          // of one channel: at most N*H*W / 4 <= S * 1024
    const int S = (int)pool_slices((long long)N * H * W);
    const dim3 grid((unsigned)S, (unsigned)C);
    hipStream_t st = tpspp::as_stream(stream);
    if (W % 4 == 0 && aligned(16, {z}) && aligned(8, {dp}))
        hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel<true>, grid, dim3(kThreads), 0, st, dp, z, mean, rstd, gamma, beta,
                           (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, windows / 2, ws);
    else
        hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel<false>, grid, dim3(kThreads), 0, st, dp, z, mean, rstd, gamma, beta,
                           (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, windows, ws);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    hipLaunchKernelGGL(bn_pool_bwd_combine_kernel, dim3((unsigned)((C + kCombine - 1) / kCombine)), dim3(kCombine), 0, st,
                       ws, S, C, sum_dr, sum_dr_x);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_bn_pool2x2_bwd_data(const float* dp, const float* z, const float* mean, const float* rstd,
                                           const float* gamma, const float* beta, const float* sum_dr,
                                           const float* sum_dr_x, int train, int N, int C, int H, int W, float* dz,
                                           tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_pool2x2_bwd_data";
    TPSPP_REQUIRE(dp && z && mean && rstd && gamma && beta && dz, "%s: null pointer", who);
    TPSPP_REQUIRE(train == 0 || train == 1, "%s: train must be 0 or 1", who);
    TPSPP_REQUIRE(!train || (sum_dr && sum_dr_x), "%s: train = 1 needs sum_dr and sum_dr_x (tpspp_bn_pool2x2_bwd_reduce)",
                  who);
    int rc = check_sizes(who, N, C, H, W);
    if (rc != TPSPP_OK || N == 0) return rc;
    const unsigned Ho = (unsigned)H / 2, Wo = (unsigned)W / 2;
    const unsigned Hc = ((unsigned)H + 1) / 2, Wc = ((unsigned)W + 1) / 2;
    const float inv_m = (float)(1.0 / ((double)N * H * W));
    hipStream_t st = tpspp::as_stream(stream);
    if (W % 4 == 0 && aligned(16, {z, dz}) && aligned(8, {dp})) {
        const unsigned units = (unsigned)N * C * Hc * (Wc / 2);
        hipLaunchKernelGGL(bn_pool_bwd_data_kernel<true>, blocks_for(units), dim3(kThreads), 0, st, dp, z, mean, rstd, gamma,
                           beta, sum_dr, sum_dr_x, train, inv_m, (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, Hc, Wc / 2,
                           units, dz);
    } else {
        const unsigned units = (unsigned)N * C * Hc * Wc;
        hipLaunchKernelGGL(bn_pool_bwd_data_kernel<false>, blocks_for(units), dim3(kThreads), 0, st, dp, z, mean, rstd, gamma,
                           beta, sum_dr, sum_dr_x, train, inv_m, (unsigned)C, (unsigned)H, (unsigned)W, Ho, Wo, Hc, Wc,
                           units, dz);
    }
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_global_avgpool_bwd(const float* g, int N, int C, int H, int W, float* dx, tpspp_stream_t stream)
{
    const char* who = "tpspp_global_avgpool_bwd";
    TPSPP_REQUIRE(g && dx, "%s: null pointer", who);
    TPSPP_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, "%s: bad sizes (N %d, C %d, H %d, W %d)", who, N, C, H, W);
    TPSPP_REQUIRE((long long)N * C * H * W <= 0x7fffffffLL, "%s: more than 2^31 - 1 elements", who);
    if (N == 0) return TPSPP_OK;
    const unsigned HW = (unsigned)H * W, total = (unsigned)N * C * HW;
    hipStream_t st = tpspp::as_stream(stream);
    if (HW % 4 == 0 && aligned(16, {dx}))
        hipLaunchKernelGGL(global_avgpool_bwd_kernel<true>, blocks_for(total / 4), dim3(kThreads), 0, st, g, HW, total, dx);
    else
        hipLaunchKernelGGL(global_avgpool_bwd_kernel<false>, blocks_for(total), dim3(kThreads), 0, st, g, HW, total, dx);
    return tpspp::check_launch(who);
}
