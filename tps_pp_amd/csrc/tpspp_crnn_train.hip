// The training kernels of the CRNN recogniser's recurrent half (include/tpspp_crnn_train.h): the LSTM recurrence that
// keeps its gates and cell states, its backward through time, and the CTC loss forward and backward on raw logits.
// Replaces: the autograd of nn.LSTM's recurrence in layers/lstm_layer.py:10,14 and torch.log_softmax + nn.CTCLoss of
// losses/ctc_loss.py:50-71 (reference).
#include "tpspp_crnn.h"
#include "tpspp_crnn_train.h"
#include "tpspp_common.h"
#include "tpspp_crnn_cell.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;
using namespace tpspp_crnn_cell;

// ---- the LSTM recurrence, saving, and its backward through time -------------------------------------------------------------
// (the two bodies and their fp32 product: tpspp_crnn_cell.h)
__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_train_kernel(const float* __restrict__ xg, const float* __restrict__ whh, float* __restrict__ out,
                       float* __restrict__ gates, float* __restrict__ cell, int T, int N, int g)
{
    lstm_forward<MulF32, true>(xg, whh, out, gates, cell, T, N, g);
}

__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ gates, const float* __restrict__ cell,
                     const float* __restrict__ wt_all, float* __restrict__ d_xg, float* __restrict__ d_xg_dir, int T, int N,
                     int g)
{
    lstm_backward<MulF32>(d_out, gates, cell, wt_all, d_xg, d_xg_dir, T, N, g);
}

constexpr size_t kBwdLds = MulF32::kBwdLds * sizeof(float);

// ---- CTC loss ------------------------------------------------------------------------------------------------------------------
constexpr int kCtcThreads = 64;             // one wavefront per image
constexpr int kReduceThreads = 256;

struct CtcParams {
    const float* logits;
    const int* targets;
    const int* target_len;
    const int* input_len;
    int N, T, C, Lmax, blank, zero_infinity, reduction;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ float lse3(float a, float b, float c)
{
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// max + log(sum exp(. - max)) of a row of C logits: every lane ends with the same bits
__device__ __forceinline__ float row_lse(const float* __restrict__ x, int C, int lane)
{
    float mx = -INFINITY;
    for (int k = lane; k < C; k += kWave) mx = fmaxf(mx, x[k]);
    mx = wave_max(mx);
    float s = 0.0f;
    for (int k = lane; k < C; k += kWave) s = s + expf(x[k] - mx);
    return mx + logf(wave_sum(s));
}

// the extended labels of image n into LDS: blank, l_1, blank, ..., l_L, blank
__device__ __forceinline__ void ctc_labels(const CtcParams& P, int n, int S, int lane, int* lab)
{
    for (int s = lane; s < S; s += kWave)
        lab[s] = (s & 1) ? clampi(P.targets[(size_t)n * P.Lmax + (s >> 1)], 0, P.C - 1) : P.blank;
}

__global__ void __launch_bounds__(kCtcThreads)
ctc_loss_fwd_kernel(const CtcParams P, float* __restrict__ loss, float* __restrict__ lse, float* __restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) int ctc_smem[];
    const int lane = threadIdx.x, n = blockIdx.x;
    const int L = clampi(P.target_len[n], 0, P.Lmax), Tn = clampi(P.input_len[n], 0, P.T);
    const int S = 2 * L + 1, Smax = 2 * P.Lmax + 1;
    int* lab = ctc_smem;
    float* prev = reinterpret_cast<float*>(ctc_smem + Smax);
    float* cur = prev + Smax;
    float* al = ws + (size_t)n * P.T * Smax;
    ctc_labels(P, n, S, lane, lab);
    __syncthreads();
    for (int t = 0; t < P.T; ++t) {
        float* arow = al + (size_t)t * Smax;
        if (t >= Tn) {                                              // past the image's length: nothing to score
            if (lane == 0) lse[(size_t)n * P.T + t] = 0.0f;
            for (int s = lane; s < Smax; s += kWave) arow[s] = -INFINITY;
            continue;
        }
        const float* x = P.logits + ((size_t)n * P.T + t) * P.C;
        const float l = row_lse(x, P.C, lane);
        if (lane == 0) lse[(size_t)n * P.T + t] = l;
        for (int s = lane; s < Smax; s += kWave) {
            float v = -INFINITY;
            if (s < S) {
                const float lp = x[lab[s]] - l;
                if (t == 0) {
                    v = s < 2 ? lp : -INFINITY;
                } else {
                    const float a = prev[s];
                    const float b = s >= 1 ? prev[s - 1] : -INFINITY;
                    const float c = (s >= 2 && lab[s] != P.blank && lab[s] != lab[s - 2]) ? prev[s - 2] : -INFINITY;
                    v = lp + lse3(a, b, c);
                }
                cur[s] = v;
            }
            arow[s] = v;
        }
        __syncthreads();
        float* tmp = prev; prev = cur; cur = tmp;
    }
    if (lane == 0) {
        float nll;
        if (Tn == 0)
            nll = L == 0 ? 0.0f : INFINITY;
        else
            nll = -lse3(prev[S - 1], S >= 2 ? prev[S - 2] : -INFINITY, -INFINITY);
        ws[(size_t)P.N * P.T * Smax + n] = nll;
        loss[n] = (P.zero_infinity && nll == INFINITY) ? 0.0f : nll;
    }
}

__global__ void __launch_bounds__(kReduceThreads)
ctc_loss_reduce_kernel(const CtcParams P, const float* __restrict__ loss, float* __restrict__ reduced)
{
    __shared__ float sS[kReduceThreads];
    float s = 0.0f;
    for (int n = threadIdx.x; n < P.N; n += kReduceThreads) {
        float v = loss[n];
        if (P.reduction == TPSPP_CTC_MEAN) {
            const int L = clampi(P.target_len[n], 0, P.Lmax);
            v = v / (float)(L > 1 ? L : 1);
        }
        s = s + v;
    }
    sS[threadIdx.x] = s;
    __syncthreads();
    for (int o = kReduceThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sS[threadIdx.x] = sS[threadIdx.x] + sS[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) reduced[0] = P.reduction == TPSPP_CTC_MEAN ? sS[0] / (float)P.N : sS[0];
}

__global__ void __launch_bounds__(kCtcThreads)
ctc_loss_bwd_kernel(const CtcParams P, const float* __restrict__ g, const float* __restrict__ lse, const float* __restrict__ ws,
                    float* __restrict__ d_logits)
{
    extern __shared__ __attribute__((aligned(16))) int ctc_smem[];
    const int lane = threadIdx.x, n = blockIdx.x;
    const int L = clampi(P.target_len[n], 0, P.Lmax), Tn = clampi(P.input_len[n], 0, P.T);
    const int S = 2 * L + 1, Smax = 2 * P.Lmax + 1;
    int* lab = ctc_smem;
    int* lead = lab + Smax;                                         // 1: no earlier state carries this state's class
    float* nxt = reinterpret_cast<float*>(lead + Smax);
    float* cur = nxt + Smax;
    float* ab = cur + Smax;                                         // alpha_t + beta_t
    float* res = ab + Smax;                                         // (C) the per-class log-sum-exp of ab
    const float* al = ws + (size_t)n * P.T * Smax;
    const float nll = ws[(size_t)P.N * P.T * Smax + n];
    float gn = P.reduction == TPSPP_CTC_NONE ? g[n] : g[0];
    if (P.reduction == TPSPP_CTC_MEAN) gn = gn / ((float)P.N * (float)(L > 1 ? L : 1));
    const bool dead = P.zero_infinity && nll == INFINITY;
    ctc_labels(P, n, S, lane, lab);
    __syncthreads();
    for (int s = lane; s < S; s += kWave) {
        int first = 1;
        for (int s2 = 0; s2 < s; ++s2)
            if (lab[s2] == lab[s]) { first = 0; break; }
        lead[s] = first;
    }
    __syncthreads();
    for (int t = P.T - 1; t >= 0; --t) {
        float* d = d_logits + ((size_t)n * P.T + t) * P.C;
        if (t >= Tn || dead) {
            for (int c = lane; c < P.C; c += kWave) d[c] = 0.0f;
            continue;
        }
        const float* x = P.logits + ((size_t)n * P.T + t) * P.C;
        const float l = lse[(size_t)n * P.T + t];
        const float* arow = al + (size_t)t * Smax;
        for (int s = lane; s < S; s += kWave) {
            const float lp = x[lab[s]] - l;
            float v;
            if (t == Tn - 1) {
                v = s >= S - 2 ? lp : -INFINITY;
            } else {
                const float a = nxt[s];
                const float b = s + 1 < S ? nxt[s + 1] : -INFINITY;
                const float c = (s + 2 < S && lab[s + 2] != P.blank && lab[s + 2] != lab[s]) ? nxt[s + 2] : -INFINITY;
                v = lp + lse3(a, b, c);
            }
            cur[s] = v;
            ab[s] = arow[s] + v;
        }
        for (int c = lane; c < P.C; c += kWave) res[c] = -INFINITY;
        __syncthreads();
        for (int s = lane; s < S; s += kWave) {
            if (!lead[s]) continue;
            const int lb = lab[s];
            float m = -INFINITY;
            for (int s2 = s; s2 < S; ++s2)
                if (lab[s2] == lb) m = fmaxf(m, ab[s2]);
            float v = -INFINITY;
            if (m != -INFINITY) {
                float sum = 0.0f;
                for (int s2 = s; s2 < S; ++s2)                      // ascending s, one lane: a fixed order
                    if (lab[s2] == lb) sum = sum + expf(ab[s2] - m);
                v = m + logf(sum);
            }
            res[lb] = v;
        }
        __syncthreads();
        for (int c = lane; c < P.C; c += kWave) {
            const float lp = x[c] - l;
            d[c] = gn * (expf(lp) - expf(res[c] - lp + nll));
        }
        __syncthreads();                                            // res and nxt are free again
        float* tmp = nxt; nxt = cur; cur = tmp;
    }
}

int check_ctc(const char* who, int N, int T, int C, int Lmax, int blank, int reduction)
{
    TPSPP_REQUIRE(N >= 0 && T >= 1, "%s: bad sizes (N >= 0, T >= 1)", who);
    TPSPP_REQUIRE(C >= 2 && C <= TPSPP_CTC_MAX_CLASSES, "%s: C must lie in [2, %d], got %d", who, TPSPP_CTC_MAX_CLASSES, C);
    TPSPP_REQUIRE(blank >= 0 && blank < C, "%s: blank %d out of range 0 .. %d", who, blank, C - 1);
    TPSPP_REQUIRE(Lmax >= 0 && Lmax <= TPSPP_CTC_MAX_TARGET, "%s: Lmax must lie in [0, %d], got %d", who, TPSPP_CTC_MAX_TARGET, Lmax);
    TPSPP_REQUIRE(reduction == TPSPP_CTC_NONE || reduction == TPSPP_CTC_MEAN || reduction == TPSPP_CTC_SUM,
                  "%s: reduction must be 0 (none), 1 (mean) or 2 (sum), got %d", who, reduction);
    TPSPP_REQUIRE((long long)N * T <= (1LL << 30), "%s: N * T too large", who);
    return TPSPP_OK;
}

CtcParams ctc_params(const float* logits, const int* targets, const int* target_len, const int* input_len, int N, int T, int C,
                     int Lmax, int blank, int zero_infinity, int reduction)
{
    CtcParams P = {};
    P.logits = logits; P.targets = targets; P.target_len = target_len; P.input_len = input_len;
    P.N = N; P.T = T; P.C = C; P.Lmax = Lmax; P.blank = blank; P.zero_infinity = zero_infinity; P.reduction = reduction;
    return P;
}

}  // namespace

TPSPP_EXPORT int tpspp_crnn_lstm_train_fwd(const float* xg, const float* w_hh, float* out, float* gates, float* cell, int T,
                                           int N, int hidden, int images_per_group, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_train_fwd";
    TPSPP_REQUIRE(xg && w_hh && out && gates && cell, "%s: null pointer", who);
    const int rc = check_lstm(who, T, N, hidden, images_per_group);
    if (rc != TPSPP_OK || N == 0) return rc;
    unsigned groups;
    const int g = lstm_grid(N, images_per_group, groups);
    if (g < 0) return g;
    hipLaunchKernelGGL(crnn_lstm_train_kernel, dim3(groups), dim3(kLstmThreads), 0, tpspp::as_stream(stream), xg, w_hh, out,
                       gates, cell, T, N, g);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_crnn_lstm_bwd(const float* d_out, const float* gates, const float* cell, const float* w_hh_t,
                                     float* d_xg, float* d_xg_dir, int T, int N, int hidden, int images_per_group,
                                     tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_bwd";
    TPSPP_REQUIRE(d_out && gates && cell && w_hh_t && d_xg, "%s: null pointer", who);
    const int rc = check_lstm(who, T, N, hidden, images_per_group);
    if (rc != TPSPP_OK || N == 0) return rc;
    unsigned groups;
    const int g = lstm_grid(N, images_per_group, groups);
    if (g < 0) return g;
    static bool attr_done[tpspp::kMaxDevices] = {};
    if (tpspp::first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&crnn_lstm_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kBwdLds);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(crnn_lstm_bwd_kernel, dim3(groups), dim3(kLstmThreads), kBwdLds, tpspp::as_stream(stream), d_out, gates,
                       cell, w_hh_t, d_xg, d_xg_dir, T, N, g);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_crnn_ctc_loss_workspace_floats(int N, int T, int Lmax)
{
    if (N <= 0 || T <= 0 || Lmax < 0) return 0;
    return (size_t)N * (size_t)T * (size_t)(2 * (size_t)Lmax + 1) + (size_t)N;
}

TPSPP_EXPORT int tpspp_crnn_ctc_loss_fwd(const float* logits, const int* targets, const int* target_len, const int* input_len,
                                         int N, int T, int C, int Lmax, int blank, int zero_infinity, int reduction, float* loss,
                                         float* lse, float* reduced, float* ws, size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_ctc_loss_fwd";
    TPSPP_REQUIRE(logits && target_len && input_len && loss && lse && ws, "%s: null pointer", who);
    int rc = check_ctc(who, N, T, C, Lmax, blank, reduction);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(targets || Lmax == 0, "%s: null pointer (targets)", who);
    TPSPP_REQUIRE(reduction == TPSPP_CTC_NONE || reduced, "%s: null pointer (reduced)", who);
    const size_t need = tpspp_crnn_ctc_loss_workspace_floats(N, T, Lmax);
    TPSPP_REQUIRE(ws_floats >= need, "%s: workspace of %zu floats, %zu needed", who, ws_floats, need);
    if (N == 0) return TPSPP_OK;
    const CtcParams P = ctc_params(logits, targets, target_len, input_len, N, T, C, Lmax, blank, zero_infinity, reduction);
    hipStream_t st = tpspp::as_stream(stream);
    const size_t lds = (size_t)3 * (2 * (size_t)Lmax + 1) * sizeof(float);
    hipLaunchKernelGGL(ctc_loss_fwd_kernel, dim3((unsigned)N), dim3(kCtcThreads), lds, st, P, loss, lse, ws);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK || reduction == TPSPP_CTC_NONE) return rc;
    hipLaunchKernelGGL(ctc_loss_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, st, P, loss, reduced);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_crnn_ctc_loss_bwd(const float* g, const float* logits, const int* targets, const int* target_len,
                                         const int* input_len, const float* lse, const float* ws, int N, int T, int C, int Lmax,
                                         int blank, int zero_infinity, int reduction, float* d_logits, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_ctc_loss_bwd";
    TPSPP_REQUIRE(g && logits && target_len && input_len && lse && ws && d_logits, "%s: null pointer", who);
    const int rc = check_ctc(who, N, T, C, Lmax, blank, reduction);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(targets || Lmax == 0, "%s: null pointer (targets)", who);
    if (N == 0) return TPSPP_OK;
    const CtcParams P = ctc_params(logits, targets, target_len, input_len, N, T, C, Lmax, blank, zero_infinity, reduction);
    const size_t lds = ((size_t)5 * (2 * (size_t)Lmax + 1) + (size_t)C) * sizeof(float);    // <= 45 KB at the limits
    hipLaunchKernelGGL(ctc_loss_bwd_kernel, dim3((unsigned)N), dim3(kCtcThreads), lds, tpspp::as_stream(stream), P, g, lse, ws,
                       d_logits);
    return tpspp::check_launch(who);
}
