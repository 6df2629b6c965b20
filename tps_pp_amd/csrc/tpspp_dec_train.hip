// Training kernels of the NRTR decoder's embedding and of the sequence cross-entropy (include/tpspp_train_dec.h; the
// decoder's attention is tpspp_attn_train.hip).
//
// replaces: the autograd of textrecog/decoders/nrtr_decoder.py:95-99 (trg_word_emb + position table) and of
// textrecog/losses/ce_loss.py (reference, mmocr/models/) in the training graph.
//
//   * embed_pos_fwd_kernel: out[b, l, :] = weight[tok[b, l], :] + pos[l, :], one thread per element.
//   * embed_bwd_slice_kernel, one workgroup per (slice of 512 tokens, class): its threads own columns and walk the slice's
//     tokens in ascending order, adding the dx rows whose token is the class; embed_bwd_reduce_kernel then adds the slices
//     in ascending order and writes every row of d_weight (zeros for the padding row).  No atomics: the order of every
//     sum is fixed by (M, num_classes, C) alone.
//   * seq_ce_fwd_kernel / seq_ce_bwd_kernel: one wavefront per (image, position), lanes over the classes; the maximum and
//     the sum of a row are reduced with a fixed butterfly, so every lane holds the same bits.  seq_ce_reduce_kernel: one
//     workgroup adds the per-position losses (thread t the positions t, t + 256, ... ascending, then a fixed tree).
#include "tpspp_common.h"
#include "tpspp_dev.h"
#include "tpspp_train_dec.h"

#include <math.h>

using namespace tpspp_dev;

namespace {

constexpr int kThreads = 256;
constexpr int kSlice = 512;       // tokens per partial sum of the embedding gradient
constexpr int kMaxK = 1024;       // classes per cross-entropy row: 16 per lane

__global__ void __launch_bounds__(kThreads)
embed_pos_fwd_kernel(const int* tok, const float* weight, const float* pos, long long total, int L, int C, int num_classes,
                     float* out)
{
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long m = idx / C;
    const int l = (int)(m % L);
    const int t = tok[m];
    const float p = pos[(long long)l * C + c];
    out[idx] = (t >= 0 && t < num_classes) ? weight[(long long)t * C + c] + p : p;
}

__global__ void __launch_bounds__(kThreads)
embed_bwd_slice_kernel(const float* dx, const int* tok, long long M, int C, int num_classes, float* ws)
{
    __shared__ int sTok[kSlice];
    const int cls = blockIdx.y;
    const long long m0 = (long long)blockIdx.x * kSlice;
    const int n = M - m0 < kSlice ? (int)(M - m0) : kSlice;
    for (int i = threadIdx.x; i < n; i += kThreads) sTok[i] = tok[m0 + i];
    __syncthreads();
    float* dst = ws + ((long long)blockIdx.x * num_classes + cls) * C;
    for (int c = threadIdx.x; c < C; c += kThreads) {
        float s = 0.0f;
        for (int i = 0; i < n; ++i)
            if (sTok[i] == cls) s = s + dx[(m0 + i) * C + c];
        dst[c] = s;
    }
}

__global__ void __launch_bounds__(kThreads)
embed_bwd_reduce_kernel(const float* ws, int slices, long long total, int C, int padding_idx, float* d_weight)
{
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;      // (class, column)
    if (idx >= total) return;
    float s = 0.0f;
    if (idx / C != padding_idx)
        for (int j = 0; j < slices; ++j) s = s + ws[(long long)j * total + idx];
    d_weight[idx] = s;
}

struct CeParams {
    const float* logits;
    const int* targets;
    long long s_n, s_l, s_k;
    int N, L, Lp, K, shift, ignore_index, reduction;
};

// the target of scored position (b, t), or -1 where the position is ignored
__device__ __forceinline__ int ce_target(const CeParams& P, int b, int t)
{
    const int y = P.targets[(long long)b * P.L + t + P.shift];
    return (y == P.ignore_index || y < 0 || y >= P.K) ? -1 : y;
}

__global__ void __launch_bounds__(kThreads)
seq_ce_fwd_kernel(const CeParams P, float* loss, float* lse_out)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);      // (b, t), t < Lp
    if (row >= (long long)P.N * P.Lp) return;
    const int b = (int)(row / P.Lp), t = (int)(row % P.Lp);
    const float* x = P.logits + b * P.s_n + t * P.s_l;
    float v[kMaxK / 64];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kMaxK / 64; ++i) {
        const int k = lane + 64 * i;
        v[i] = k < P.K ? x[k * P.s_k] : -INFINITY;
        mx = fmaxf(mx, v[i]);
    }
    mx = wave_max(mx);
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < kMaxK / 64; ++i)
        if (lane + 64 * i < P.K) s = s + expf(v[i] - mx);
    const float lse = mx + logf(wave_sum(s));
    if (lane == 0) {
        const int y = ce_target(P, b, t);
        lse_out[row] = lse;
        loss[row] = y >= 0 ? lse - x[y * P.s_k] : 0.0f;
    }
}

__global__ void __launch_bounds__(kThreads)
seq_ce_reduce_kernel(const CeParams P, const float* loss, float* reduced, float* count)
{
    __shared__ float sS[kThreads], sC[kThreads];
    const long long rows = (long long)P.N * P.Lp;
    float s = 0.0f, c = 0.0f;
    for (long long r = threadIdx.x; r < rows; r += kThreads) {
        s = s + loss[r];
        c = c + (ce_target(P, (int)(r / P.Lp), (int)(r % P.Lp)) >= 0 ? 1.0f : 0.0f);
    }
    sS[threadIdx.x] = s;
    sC[threadIdx.x] = c;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            sS[threadIdx.x] = sS[threadIdx.x] + sS[threadIdx.x + o];
            sC[threadIdx.x] = sC[threadIdx.x] + sC[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        count[0] = sC[0];
        reduced[0] = P.reduction == TPSPP_CE_MEAN ? sS[0] / sC[0] : sS[0];      // 0 / 0 = NaN, as PyTorch
    }
}

__global__ void __launch_bounds__(kThreads)
seq_ce_bwd_kernel(const CeParams P, const float* g, const float* lse, const float* count, float* d_logits)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);      // (b, t), t < L
    if (row >= (long long)P.N * P.L) return;
    const int b = (int)(row / P.L), t = (int)(row % P.L);
    float* d = d_logits + row * P.K;
    const int y = t < P.Lp ? ce_target(P, b, t) : -1;
    if (y < 0) {                      // ignored, or the position the shift drops: exact zeros, nothing read
        for (int k = lane; k < P.K; k += 64) d[k] = 0.0f;
        return;
    }
    const long long r = (long long)b * P.Lp + t;
    float gr = P.reduction == TPSPP_CE_NONE ? g[r] : g[0];
    if (P.reduction == TPSPP_CE_MEAN) gr = gr / count[0];
    const float* x = P.logits + b * P.s_n + t * P.s_l;
    const float l = lse[r];
    for (int k = lane; k < P.K; k += 64) d[k] = (expf(x[k * P.s_k] - l) - (k == y ? 1.0f : 0.0f)) * gr;
}

int check_ce(const char* who, int N, int L, int K, int shift, int reduction)
{
    TPSPP_REQUIRE(N >= 0 && L > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(K >= 1 && K <= kMaxK, "%s: K must lie in [1, %d], got %d", who, kMaxK, K);
    TPSPP_REQUIRE(shift == 0 || shift == 1, "%s: shift must be 0 or 1, got %d", who, shift);
    TPSPP_REQUIRE(reduction == TPSPP_CE_NONE || reduction == TPSPP_CE_MEAN || reduction == TPSPP_CE_SUM,
                  "%s: reduction must be 0 (none), 1 (mean) or 2 (sum), got %d", who, reduction);
    TPSPP_REQUIRE(((long long)N * L + 3) / 4 <= 0x7fffffffLL, "%s: grid too large", who);
    return TPSPP_OK;
}

CeParams ce_params(const float* logits, long long s_n, long long s_l, long long s_k, const int* targets, int N, int L, int K,
                   int shift, int ignore_index, int reduction)
{
    CeParams P = {};
    P.logits = logits; P.targets = targets; P.s_n = s_n; P.s_l = s_l; P.s_k = s_k;
    P.N = N; P.L = L; P.Lp = L - shift; P.K = K; P.shift = shift; P.ignore_index = ignore_index; P.reduction = reduction;
    return P;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
TPSPP_EXPORT int tpspp_embed_pos_fwd(const int* tok, const float* weight, const float* pos, int N, int L, int C,
                                     int num_classes, float* out, tpspp_stream_t stream)
{
    const char* who = "tpspp_embed_pos_fwd";
    TPSPP_REQUIRE(tok && weight && pos && out, "%s: null pointer", who);
    TPSPP_REQUIRE(N >= 0 && L > 0 && C > 0 && num_classes > 0, "%s: bad sizes", who);
    const long long total = (long long)N * L * C;
    TPSPP_REQUIRE((total + kThreads - 1) / kThreads <= 0x7fffffffLL, "%s: grid too large", who);
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(embed_pos_fwd_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       tpspp::as_stream(stream), tok, weight, pos, total, L, C, num_classes, out);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_embed_bwd_workspace_floats(long long M, int num_classes, int C)
{
    if (M <= 0 || num_classes <= 0 || C <= 0) return 0;
    return (size_t)((M + kSlice - 1) / kSlice) * (size_t)num_classes * (size_t)C;
}

TPSPP_EXPORT int tpspp_embed_bwd(const float* dx, const int* tok, long long M, int C, int num_classes, int padding_idx,
                                 float* d_weight, float* ws, size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_embed_bwd";
    TPSPP_REQUIRE(dx && tok && d_weight && ws, "%s: null pointer", who);
    TPSPP_REQUIRE(M >= 0 && C > 0 && num_classes > 0 && num_classes <= 65535, "%s: bad sizes", who);
    const long long slices = (M + kSlice - 1) / kSlice, total = (long long)num_classes * C;
    TPSPP_REQUIRE(slices <= 0x7fffffffLL && (total + kThreads - 1) / kThreads <= 0x7fffffffLL, "%s: grid too large", who);
    TPSPP_REQUIRE(ws_floats >= tpspp_embed_bwd_workspace_floats(M, num_classes, C),
                  "%s: workspace of %zu floats, %zu needed", who, ws_floats, tpspp_embed_bwd_workspace_floats(M, num_classes, C));
    if (M == 0) return TPSPP_OK;
    hipStream_t st = tpspp::as_stream(stream);
    hipLaunchKernelGGL(embed_bwd_slice_kernel, dim3((unsigned)slices, (unsigned)num_classes), dim3(kThreads), 0, st, dx, tok, M,
                       C, num_classes, ws);
    const int rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    hipLaunchKernelGGL(embed_bwd_reduce_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws,
                       (int)slices, total, C, padding_idx, d_weight);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_seq_ce_fwd(const float* logits, long long s_n, long long s_l, long long s_k, const int* targets, int N,
                                  int L, int K, int shift, int ignore_index, int reduction, float* loss, float* lse,
                                  float* reduced, float* count, tpspp_stream_t stream)
{
    const char* who = "tpspp_seq_ce_fwd";
    TPSPP_REQUIRE(logits && targets && loss && lse, "%s: null pointer", who);
    int rc = check_ce(who, N, L, K, shift, reduction);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(reduction == TPSPP_CE_NONE || (reduced && count), "%s: null pointer (reduced / count)", who);
    if (N == 0) return TPSPP_OK;
    const CeParams P = ce_params(logits, s_n, s_l, s_k, targets, N, L, K, shift, ignore_index, reduction);
    hipStream_t st = tpspp::as_stream(stream);
    const long long rows = (long long)N * P.Lp;
    if (rows > 0) {
        hipLaunchKernelGGL(seq_ce_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kThreads), 0, st, P, loss, lse);
        rc = tpspp::check_launch(who);
        if (rc != TPSPP_OK) return rc;
    }
    if (reduction == TPSPP_CE_NONE) return TPSPP_OK;
    hipLaunchKernelGGL(seq_ce_reduce_kernel, dim3(1), dim3(kThreads), 0, st, P, loss, reduced, count);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_seq_ce_bwd(const float* g, const float* logits, long long s_n, long long s_l, long long s_k,
                                  const int* targets, const float* lse, const float* count, int N, int L, int K, int shift,
                                  int ignore_index, int reduction, float* d_logits, tpspp_stream_t stream)
{
    const char* who = "tpspp_seq_ce_bwd";
    TPSPP_REQUIRE(g && logits && targets && lse && d_logits, "%s: null pointer", who);
    const int rc = check_ce(who, N, L, K, shift, reduction);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(reduction != TPSPP_CE_MEAN || count, "%s: null pointer (count)", who);
    if (N == 0) return TPSPP_OK;
    const CeParams P = ce_params(logits, s_n, s_l, s_k, targets, N, L, K, shift, ignore_index, reduction);
    hipLaunchKernelGGL(seq_ce_bwd_kernel, dim3((unsigned)(((long long)N * L + 3) / 4)), dim3(kThreads), 0,
                       tpspp::as_stream(stream), P, g, lse, count, d_logits);
    return tpspp::check_launch(who);
}
