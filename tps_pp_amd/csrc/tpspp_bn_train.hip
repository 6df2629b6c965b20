// BatchNorm in training mode, fused with the residual add and the ReLU that follow it in a BasicBlock: the kernels of the
// backbone's training graph (ResNetABI_v2_large.set_train_backend("hip")).  fp32, NCHW, per channel over M = N*H*W.
//
//   * bn_stats_kernel + bn_stats_combine_kernel: per-channel mean and biased variance.  FIXED SPLIT: the M elements of a
//     channel are cut into S = ceil(M / 4096) slices; a workgroup holds its slice in registers (16 elements per thread),
//     forms the slice's mean and then the sum of squared deviations from it (two passes over registers: no E[z^2] - E[z]^2
//     cancellation), and writes (count, mean, M2) to the caller's workspace.  The combine launch merges the slices in slice
//     order with Chan's formula in fp64, forms rstd = 1 / sqrt(var + eps) and, when asked, updates the running statistics
//     with PyTorch's rule (unbiased variance, momentum or the cumulative 1 / num_batches_tracked).
//   * bn_apply_kernel: y = relu(g_a (z_a - mu_a) rstd_a + b_a + r), r = nothing, a residual tensor, or a second normalised
//     branch g_b (z_b - mu_b) rstd_b + b_b (the downsample shortcut).  One pass, float4 when H*W % 4 == 0.
//   * bn_bwd_reduce_kernel + bn_bwd_reduce_combine_kernel: dr = dy [y > 0] (the mask read from the saved output) and, per
//     channel, sum dr, sum dr xhat_a, sum dr xhat_b: the beta and gamma gradients.  Same fixed split, slices added in
//     slice order in fp64.
//   * bn_bwd_data_kernel: dz = g rstd (dr - sum dr / M - xhat sum dr xhat / M) for a training-mode BN, g rstd dr for an
//     eval-mode one (xhat recomputed from z, mu, rstd), for one or both branches; optionally the shortcut's gradient dr,
//     written or added into a given gradient.
// No atomics anywhere: results are bitwise identical from call to call and from stream to stream.  No allocation and no
// host synchronisation in the entry points; workspaces come from the caller.
//
// Replaces (reference, mmocr/models/textrecog/): nn.BatchNorm2d (training mode, running statistics), the residual add and
// nn.ReLU of backbones/resnet_v2_large.py and layers/conv_layer.py:12-33, forward and autograd.
#include "tpspp_common.h"
#include "tpspp_dev.h"

#include <math.h>

#include <initializer_list>

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 16;                          // elements of the channel per thread and slice
constexpr int kSlice = kThreads * kPer;           // 4096 elements per slice
constexpr int kCombine = 64;                      // threads of a combine workgroup (one per channel)

inline long long bn_slices(long long M) { return (M + kSlice - 1) / kSlice; }

// offset of element m (0 <= m < M) of channel c in an NCHW tensor
__device__ __forceinline__ unsigned chan_off(unsigned m, unsigned C, unsigned HW, unsigned c)
{
    const unsigned n = m / HW;
    return (n * C + c) * HW + (m - n * HW);
}

using tpspp_dev::block_sums;

// ------------------------------------------------------------------------------------------------------------------
// statistics: slice s of channel c -> ws[(s * C + c) * 3 + {0, 1, 2}] = (count, mean, M2)
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_stats_kernel(const float* __restrict__ z, unsigned C, unsigned HW, unsigned M, float* __restrict__ ws)
{
    __shared__ float red[2][4];
    const unsigned s = blockIdx.x, c = blockIdx.y;
    const unsigned m0 = s * (unsigned)kSlice;
    const unsigned cnt = min((unsigned)kSlice, M - m0);
    float v[kPer];
    float sum[1] = {0.0f};
    if (VEC) {
#pragma unroll
        for (int j = 0; j < kPer / 4; ++j) {
            const unsigned m = m0 + (unsigned)(j * kThreads + threadIdx.x) * 4u;
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < M) q = *reinterpret_cast<const float4*>(z + chan_off(m, C, HW, c));
            v[4 * j] = q.x; v[4 * j + 1] = q.y; v[4 * j + 2] = q.z; v[4 * j + 3] = q.w;
            sum[0] = sum[0] + ((q.x + q.y) + (q.z + q.w));
        }
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const unsigned m = m0 + (unsigned)(j * kThreads + threadIdx.x);
            v[j] = m < M ? z[chan_off(m, C, HW, c)] : 0.0f;
            sum[0] = sum[0] + v[j];
        }
    }
    block_sums<1>(sum, red);
    const float mu = sum[0] / (float)cnt;
    float q2[1] = {0.0f};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const unsigned m = VEC ? m0 + (unsigned)((j / 4) * kThreads + threadIdx.x) * 4u + (unsigned)(j % 4)
                               : m0 + (unsigned)(j * kThreads + threadIdx.x);
        const float d = m < M ? v[j] - mu : 0.0f;
        q2[0] = q2[0] + d * d;
    }
    block_sums<1>(q2, red);
    if (threadIdx.x == 0) {
        float* w = ws + ((size_t)s * C + c) * 3;
        w[0] = (float)cnt;
        w[1] = mu;
        w[2] = q2[0];
    }
}

// slices merged in slice order (Chan et al.), fp64; mean / rstd out, running statistics updated when rm != NULL
__global__ void __launch_bounds__(kCombine)
bn_stats_combine_kernel(const float* __restrict__ ws, int S, int C, float eps, float momentum,
                        const long long* __restrict__ nbt, float* __restrict__ rm, float* __restrict__ rv,
                        float* __restrict__ mean, float* __restrict__ rstd)
{
    __shared__ float sh[3][kCombine];
    const int c = blockIdx.x, lane = threadIdx.x;
    double n = 0.0, mu = 0.0, m2 = 0.0;
    for (int s0 = 0; s0 < S; s0 += kCombine) {
        const int s = s0 + lane;
        if (s < S) {
            const float* w = ws + ((size_t)s * C + c) * 3;
            sh[0][lane] = w[0]; sh[1][lane] = w[1]; sh[2][lane] = w[2];
        }
        __syncthreads();
        if (lane == 0) {
            const int k1 = min(kCombine, S - s0);
            for (int k = 0; k < k1; ++k) {
                const double nb = sh[0][k], mb = sh[1][k], qb = sh[2][k];
                const double nn = n + nb;
                const double d = mb - mu;
                mu = mu + d * (nb / nn);
                m2 = m2 + qb + d * d * (n * nb / nn);
                n = nn;
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    const double var = m2 / n;
    mean[c] = (float)mu;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (rm != nullptr) {
        const double f = momentum >= 0.0f ? (double)momentum : 1.0 / (double)(nbt[0] + 1);
        const double unb = n > 1.0 ? var * (n / (n - 1.0)) : var;
        rm[c] = (float)((1.0 - f) * (double)rm[c] + f * mu);
        rv[c] = (float)((1.0 - f) * (double)rv[c] + f * unb);
    }
}

// num_batches_tracked += 1 (its own launch: every combine workgroup has read the old value by then)
__global__ void __launch_bounds__(64) bn_count_kernel(long long* __restrict__ nbt)
{
    if (threadIdx.x == 0) nbt[0] = nbt[0] + 1;
}

__global__ void __launch_bounds__(kThreads)
bn_eval_stats_kernel(const float* __restrict__ rm, const float* __restrict__ rv, int C, float eps, float* __restrict__ mean,
                     float* __restrict__ rstd)
{
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    mean[c] = rm[c];
    rstd[c] = (float)(1.0 / sqrt((double)rv[c] + (double)eps));
}

// ------------------------------------------------------------------------------------------------------------------
struct Branch {
    const float* z;
    const float* mean;
    const float* rstd;
    const float* gamma;
    const float* beta;      // forward: beta; backward: sum dr xhat of this branch
    float* dz;              // backward only
    int train;              // backward only
};

// y = relu(g_a (z_a - mu_a) rstd_a + b_a + r); res_mode 0 none, 1 residual tensor r, 2 branch b
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_apply_kernel(const Branch a, const Branch b, const float* __restrict__ r, int res_mode, int relu, unsigned C,
                unsigned HW, unsigned total, float* __restrict__ y)
{
    constexpr int W = VEC ? 4 : 1;
    const unsigned e = (blockIdx.x * (unsigned)kThreads + threadIdx.x) * (unsigned)W;
    if (e >= total) return;
    const unsigned c = (e / HW) % C;
    const float mua = a.mean[c], sa = a.gamma[c] * a.rstd[c], ba = a.beta[c];
    float zv[W], out[W];
    if (VEC) *reinterpret_cast<float4*>(zv) = *reinterpret_cast<const float4*>(a.z + e);
    else zv[0] = a.z[e];
#pragma unroll
    for (int i = 0; i < W; ++i) out[i] = (zv[i] - mua) * sa + ba;
    if (res_mode == 1) {
        float rv[W];
        if (VEC) *reinterpret_cast<float4*>(rv) = *reinterpret_cast<const float4*>(r + e);
        else rv[0] = r[e];
#pragma unroll
        for (int i = 0; i < W; ++i) out[i] = out[i] + rv[i];
    } else if (res_mode == 2) {
        const float mub = b.mean[c], sb = b.gamma[c] * b.rstd[c], bb = b.beta[c];
        float zb[W];
        if (VEC) *reinterpret_cast<float4*>(zb) = *reinterpret_cast<const float4*>(b.z + e);
        else zb[0] = b.z[e];
#pragma unroll
        for (int i = 0; i < W; ++i) out[i] = out[i] + ((zb[i] - mub) * sb + bb);
    }
    if (relu) {
#pragma unroll
        for (int i = 0; i < W; ++i) out[i] = out[i] > 0.0f ? out[i] : 0.0f;
    }
    if (VEC) *reinterpret_cast<float4*>(y + e) = *reinterpret_cast<const float4*>(out);
    else y[e] = out[0];
}

// ------------------------------------------------------------------------------------------------------------------
// backward reduction: slice s of channel c -> ws[(s * C + c) * 3 + {0, 1, 2}] = (sum dr, sum dr xhat_a, sum dr xhat_b)
template <bool VEC, bool TWO>
__global__ void __launch_bounds__(kThreads)
bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ y, int relu, const Branch a, const Branch b,
                     unsigned C, unsigned HW, unsigned M, float* __restrict__ ws)
{
    __shared__ float red[3][4];
    constexpr int W = VEC ? 4 : 1;
    const unsigned s = blockIdx.x, c = blockIdx.y;
    const unsigned m0 = s * (unsigned)kSlice;
    const float mua = a.mean[c], ra = a.rstd[c];
    const float mub = TWO ? b.mean[c] : 0.0f, rb = TWO ? b.rstd[c] : 0.0f;
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < kPer / W; ++j) {
        const unsigned m = m0 + (unsigned)(j * kThreads + threadIdx.x) * (unsigned)W;
        if (m >= M) continue;
        const unsigned o = chan_off(m, C, HW, c);
        float g[W], t[W] = {}, za[W], zb[W] = {};
        if (VEC) {
            *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(dy + o);
            *reinterpret_cast<float4*>(za) = *reinterpret_cast<const float4*>(a.z + o);
            if (relu) *reinterpret_cast<float4*>(t) = *reinterpret_cast<const float4*>(y + o);
            if (TWO) *reinterpret_cast<float4*>(zb) = *reinterpret_cast<const float4*>(b.z + o);
        } else {
            g[0] = dy[o];
            za[0] = a.z[o];
            if (relu) t[0] = y[o];
            if (TWO) zb[0] = b.z[o];
        }
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float dr = (relu && !(t[i] > 0.0f)) ? 0.0f : g[i];
            acc[0] = acc[0] + dr;
            acc[1] = acc[1] + dr * ((za[i] - mua) * ra);
            if (TWO) acc[2] = acc[2] + dr * ((zb[i] - mub) * rb);
        }
    }
    block_sums<3>(acc, red);
    if (threadIdx.x == 0) {
        float* w = ws + ((size_t)s * C + c) * 3;
        w[0] = acc[0];
        w[1] = acc[1];
        w[2] = acc[2];
    }
}

__global__ void __launch_bounds__(kCombine)
bn_bwd_reduce_combine_kernel(const float* __restrict__ ws, int S, int C, float* __restrict__ s_dr, float* __restrict__ s_xa,
                             float* __restrict__ s_xb)
{
    __shared__ float sh[3][kCombine];
    const int c = blockIdx.x, lane = threadIdx.x;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int s0 = 0; s0 < S; s0 += kCombine) {
        const int s = s0 + lane;
        if (s < S) {
            const float* w = ws + ((size_t)s * C + c) * 3;
            sh[0][lane] = w[0]; sh[1][lane] = w[1]; sh[2][lane] = w[2];
        }
        __syncthreads();
        if (lane == 0) {
            const int k1 = min(kCombine, S - s0);
            for (int k = 0; k < k1; ++k) {
                t0 = t0 + (double)sh[0][k];
                t1 = t1 + (double)sh[1][k];
                t2 = t2 + (double)sh[2][k];
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    s_dr[c] = (float)t0;
    s_xa[c] = (float)t1;
    if (s_xb != nullptr) s_xb[c] = (float)t2;
}

// ------------------------------------------------------------------------------------------------------------------
// dz_a / dz_b from dr = dy [y > 0]; dres: 1 written with dr, 2 dr added into it
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
bn_bwd_data_kernel(const float* __restrict__ dy, const float* __restrict__ y, int relu, const Branch a, const Branch b,
                   const float* __restrict__ s_dr, float inv_m, float* __restrict__ dres, int dres_mode, unsigned C,
                   unsigned HW, unsigned total)
{
    constexpr int W = VEC ? 4 : 1;
    const unsigned e = (blockIdx.x * (unsigned)kThreads + threadIdx.x) * (unsigned)W;
    if (e >= total) return;
    const unsigned c = (e / HW) % C;
    float dr[W];
    if (VEC) *reinterpret_cast<float4*>(dr) = *reinterpret_cast<const float4*>(dy + e);
    else dr[0] = dy[e];
    if (relu) {
        float t[W];
        if (VEC) *reinterpret_cast<float4*>(t) = *reinterpret_cast<const float4*>(y + e);
        else t[0] = y[e];
#pragma unroll
        for (int i = 0; i < W; ++i) dr[i] = t[i] > 0.0f ? dr[i] : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const Branch& q = p == 0 ? a : b;
        if (q.dz == nullptr) continue;
        const float mu = q.mean[c], rs = q.rstd[c], sc = q.gamma[c] * rs;
        float out[W];
        if (q.train) {
            // the sums exist only for a training-mode branch (an eval-mode one may come with sum_dr == NULL)
            const float k0 = s_dr[c] * inv_m;
            const float k1 = q.beta[c] * inv_m;
            float zv[W];
            if (VEC) *reinterpret_cast<float4*>(zv) = *reinterpret_cast<const float4*>(q.z + e);
            else zv[0] = q.z[e];
#pragma unroll
            for (int i = 0; i < W; ++i) out[i] = sc * ((dr[i] - k0) - ((zv[i] - mu) * rs) * k1);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) out[i] = sc * dr[i];
        }
        if (VEC) *reinterpret_cast<float4*>(q.dz + e) = *reinterpret_cast<const float4*>(out);
        else q.dz[e] = out[0];
    }
    if (dres_mode == 2) {
        float o[W];
        if (VEC) *reinterpret_cast<float4*>(o) = *reinterpret_cast<const float4*>(dres + e);
        else o[0] = dres[e];
#pragma unroll
        for (int i = 0; i < W; ++i) dr[i] = o[i] + dr[i];
    }
    if (dres_mode != 0) {
        if (VEC) *reinterpret_cast<float4*>(dres + e) = *reinterpret_cast<const float4*>(dr);
        else dres[e] = dr[0];
    }
}

// the float4 forms need H*W % 4 == 0 and 16-byte aligned tensors (a view may start anywhere)
bool vec_ok(int HW, std::initializer_list<const void*> ptrs)
{
    if (HW % 4 != 0) return false;
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
    return true;
}

int check_sizes(const char* who, int N, int C, int HW)
{
    TPSPP_REQUIRE(N >= 0 && C > 0 && HW > 0, "%s: bad sizes (N %d, C %d, H*W %d)", who, N, C, HW);
    TPSPP_REQUIRE((long long)N * C * HW <= 0x7fffffffLL, "%s: more than 2^31 - 1 elements", who);
    TPSPP_REQUIRE(C <= 65535 && bn_slices((long long)N * HW) <= 0x7fffffffLL, "%s: grid too large", who);
    return TPSPP_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
TPSPP_EXPORT size_t tpspp_bn_stats_workspace_floats(int N, int C, int HW)
{
    if (N <= 0 || C <= 0 || HW <= 0) return 0;
    return (size_t)bn_slices((long long)N * HW) * (size_t)C * 3;
}

TPSPP_EXPORT int tpspp_bn_train_stats(const float* z, int N, int C, int HW, float eps, float momentum,
                                      long long* num_batches_tracked, float* running_mean, float* running_var, float* mean,
                                      float* rstd, float* ws, size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_train_stats";
    TPSPP_REQUIRE(z && mean && rstd, "%s: null pointer", who);
    int rc = check_sizes(who, N, C, HW);
    if (rc != TPSPP_OK) return rc;
    const long long M = (long long)N * HW;
    TPSPP_REQUIRE(M >= 1, "%s: batch statistics of an empty batch", who);
    TPSPP_REQUIRE(eps >= 0.0f, "%s: eps must be >= 0", who);
    TPSPP_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
                  "%s: running_mean and running_var are given together or not at all", who);
    const bool update = running_mean != nullptr;
    TPSPP_REQUIRE(!update || M >= 2, "%s: the running variance needs more than 1 value per channel (M = %lld)", who, M);
    TPSPP_REQUIRE(!update || momentum >= 0.0f || num_batches_tracked,
                  "%s: momentum < 0 (cumulative average) needs num_batches_tracked", who);
    TPSPP_REQUIRE(momentum <= 1.0f, "%s: momentum must be <= 1", who);
    const size_t need = tpspp_bn_stats_workspace_floats(N, C, HW);
    TPSPP_REQUIRE(ws_floats >= need && ws,
                  "%s: ws too small (needs tpspp_bn_stats_workspace_floats(...) = %zu floats, got %zu)", who, need,
                  ws_floats);
    hipStream_t st = tpspp::as_stream(stream);
    const int S = (int)bn_slices(M);
    const dim3 grid((unsigned)S, (unsigned)C);
    if (vec_ok(HW, {z}))
        hipLaunchKernelGGL(bn_stats_kernel<true>, grid, dim3(kThreads), 0, st, z, (unsigned)C, (unsigned)HW, (unsigned)M, ws);
    else
        hipLaunchKernelGGL(bn_stats_kernel<false>, grid, dim3(kThreads), 0, st, z, (unsigned)C, (unsigned)HW, (unsigned)M, ws);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    hipLaunchKernelGGL(bn_stats_combine_kernel, dim3((unsigned)C), dim3(kCombine), 0, st, ws, S, C, eps, momentum,
                       update ? num_batches_tracked : nullptr, running_mean, running_var, mean, rstd);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK || !update || num_batches_tracked == nullptr) return rc;
    hipLaunchKernelGGL(bn_count_kernel, dim3(1), dim3(64), 0, st, num_batches_tracked);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps, float* mean,
                                     float* rstd, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_eval_stats";
    TPSPP_REQUIRE(running_mean && running_var && mean && rstd, "%s: null pointer", who);
    TPSPP_REQUIRE(C > 0, "%s: bad size", who);
    TPSPP_REQUIRE(eps >= 0.0f, "%s: eps must be >= 0", who);
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       tpspp::as_stream(stream), running_mean, running_var, C, eps, mean, rstd);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_bn_apply_fwd(const float* za, const float* mean_a, const float* rstd_a, const float* gamma_a,
                                    const float* beta_a, int res_mode, const float* residual, const float* zb,
                                    const float* mean_b, const float* rstd_b, const float* gamma_b, const float* beta_b,
                                    int relu, int N, int C, int HW, float* y, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_apply_fwd";
    TPSPP_REQUIRE(za && mean_a && rstd_a && gamma_a && beta_a && y, "%s: null pointer", who);
    TPSPP_REQUIRE(res_mode >= 0 && res_mode <= 2, "%s: res_mode must be 0 (none), 1 (residual) or 2 (second branch)", who);
    TPSPP_REQUIRE(res_mode != 1 || residual, "%s: null pointer (residual)", who);
    TPSPP_REQUIRE(res_mode != 2 || (zb && mean_b && rstd_b && gamma_b && beta_b), "%s: null pointer (branch b)", who);
    TPSPP_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    int rc = check_sizes(who, N, C, HW);
    if (rc != TPSPP_OK || N == 0) return rc;
    const Branch a{za, mean_a, rstd_a, gamma_a, beta_a, nullptr, 0};
    const Branch b{zb, mean_b, rstd_b, gamma_b, beta_b, nullptr, 0};
    const unsigned total = (unsigned)((long long)N * C * HW);
    hipStream_t st = tpspp::as_stream(stream);
    if (vec_ok(HW, {za, y, residual, zb}))
        hipLaunchKernelGGL(bn_apply_kernel<true>, dim3((total / 4 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a, b,
                           residual, res_mode, relu, (unsigned)C, (unsigned)HW, total, y);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, st, a, b,
                           residual, res_mode, relu, (unsigned)C, (unsigned)HW, total, y);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_bn_bwd_reduce_workspace_floats(int N, int C, int HW)
{
    return tpspp_bn_stats_workspace_floats(N, C, HW);
}

TPSPP_EXPORT int tpspp_bn_bwd_reduce(const float* dy, const float* y, int relu, const float* za, const float* mean_a,
                                     const float* rstd_a, const float* zb, const float* mean_b, const float* rstd_b, int N,
                                     int C, int HW, float* sum_dr, float* sum_dr_xa, float* sum_dr_xb, float* ws,
                                     size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_bwd_reduce";
    TPSPP_REQUIRE(dy && za && mean_a && rstd_a && sum_dr && sum_dr_xa, "%s: null pointer", who);
    TPSPP_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    TPSPP_REQUIRE(!relu || y, "%s: relu = 1 needs the forward's output y (the mask is y > 0)", who);
    const bool two = zb != nullptr;
    TPSPP_REQUIRE(!two || (mean_b && rstd_b && sum_dr_xb), "%s: null pointer (branch b)", who);
    TPSPP_REQUIRE(two || !sum_dr_xb, "%s: sum_dr_xb given without branch b", who);
    int rc = check_sizes(who, N, C, HW);
    if (rc != TPSPP_OK) return rc;
    const size_t need = tpspp_bn_bwd_reduce_workspace_floats(N, C, HW);
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_bn_bwd_reduce_workspace_floats(...) = %zu floats, got %zu)", who, need,
                  ws_floats);
    hipStream_t st = tpspp::as_stream(stream);
    const long long M = (long long)N * HW;
    if (M == 0) {
        // an empty batch: every sum is 0 (the combine launch with no slices writes them)
        hipLaunchKernelGGL(bn_bwd_reduce_combine_kernel, dim3((unsigned)C), dim3(kCombine), 0, st, ws, 0, C, sum_dr,
                           sum_dr_xa, sum_dr_xb);
        return tpspp::check_launch(who);
    }
    const Branch a{za, mean_a, rstd_a, nullptr, nullptr, nullptr, 0};
    const Branch b{zb, mean_b, rstd_b, nullptr, nullptr, nullptr, 0};
    const int S = (int)bn_slices(M);
    const dim3 grid((unsigned)S, (unsigned)C);
    const bool vec = vec_ok(HW, {dy, y, za, zb});
    if (vec && two)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<true, true>), grid, dim3(kThreads), 0, st, dy, y, relu, a, b, (unsigned)C,
                           (unsigned)HW, (unsigned)M, ws);
    else if (vec)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<true, false>), grid, dim3(kThreads), 0, st, dy, y, relu, a, b, (unsigned)C,
                           (unsigned)HW, (unsigned)M, ws);
    else if (two)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<false, true>), grid, dim3(kThreads), 0, st, dy, y, relu, a, b, (unsigned)C,
                           (unsigned)HW, (unsigned)M, ws);
    else
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<false, false>), grid, dim3(kThreads), 0, st, dy, y, relu, a, b, (unsigned)C,
                           (unsigned)HW, (unsigned)M, ws);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    hipLaunchKernelGGL(bn_bwd_reduce_combine_kernel, dim3((unsigned)C), dim3(kCombine), 0, st, ws, S, C, sum_dr, sum_dr_xa,
                       sum_dr_xb);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_bn_bwd_data(const float* dy, const float* y, int relu, const float* za, const float* mean_a,
                                   const float* rstd_a, const float* gamma_a, const float* sum_dr_xa, int train_a, float* dza,
                                   const float* zb, const float* mean_b, const float* rstd_b, const float* gamma_b,
                                   const float* sum_dr_xb, int train_b, float* dzb, const float* sum_dr, float* dres,
                                   int dres_mode, int N, int C, int HW, tpspp_stream_t stream)
{
    const char* who = "tpspp_bn_bwd_data";
    TPSPP_REQUIRE(dy, "%s: null pointer (dy)", who);
    TPSPP_REQUIRE(relu == 0 || relu == 1, "%s: relu must be 0 or 1", who);
    TPSPP_REQUIRE(!relu || y, "%s: relu = 1 needs the forward's output y (the mask is y > 0)", who);
    TPSPP_REQUIRE(train_a == 0 || train_a == 1, "%s: train_a must be 0 or 1", who);
    TPSPP_REQUIRE(train_b == 0 || train_b == 1, "%s: train_b must be 0 or 1", who);
    TPSPP_REQUIRE(dres_mode >= 0 && dres_mode <= 2, "%s: dres_mode must be 0 (none), 1 (write dr) or 2 (add dr)", who);
    TPSPP_REQUIRE(dres_mode == 0 || dres, "%s: null pointer (dres)", who);
    TPSPP_REQUIRE(dza || dzb || dres_mode != 0, "%s: nothing to compute (dza, dzb NULL and dres_mode 0)", who);
    TPSPP_REQUIRE(!dza || (za && mean_a && rstd_a && gamma_a && (!train_a || (sum_dr_xa && sum_dr))),
                  "%s: null pointer (branch a)", who);
    TPSPP_REQUIRE(!dzb || (zb && mean_b && rstd_b && gamma_b && (!train_b || (sum_dr_xb && sum_dr))),
                  "%s: null pointer (branch b)", who);
    int rc = check_sizes(who, N, C, HW);
    if (rc != TPSPP_OK || N == 0) return rc;
    const Branch a{za, mean_a, rstd_a, gamma_a, sum_dr_xa, dza, train_a};
    const Branch b{zb, mean_b, rstd_b, gamma_b, sum_dr_xb, dzb, train_b};
    const unsigned total = (unsigned)((long long)N * C * HW);
    const float inv_m = (float)(1.0 / ((double)N * HW));
    hipStream_t st = tpspp::as_stream(stream);
    if (vec_ok(HW, {dy, y, za, dza, zb, dzb, dres}))
        hipLaunchKernelGGL(bn_bwd_data_kernel<true>, dim3((total / 4 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, dy,
                           y, relu, a, b, sum_dr, inv_m, dres, dres_mode, (unsigned)C, (unsigned)HW, total);
    else
        hipLaunchKernelGGL(bn_bwd_data_kernel<false>, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, st, dy, y,
                           relu, a, b, sum_dr, inv_m, dres, dres_mode, (unsigned)C, (unsigned)HW, total);
    return tpspp::check_launch(who);
}
