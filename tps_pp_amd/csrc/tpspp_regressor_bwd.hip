// Training kernels of the control-point regressor's non-convolution layers (train backend "hip_all"): DGAB, the
// attention score, CBAM and the localization FCs, forward and backward, fp32.
//
// The blocks are composed (tps_pp_amd/ops.py: dgab_autograd, score_autograd, cbam_autograd, tpe_points_autograd) from
// a small set of kernels:
//   * mm_kernel: every Linear layer's forward and data gradient and the score's three batched products.  A strided,
//     batched C[b][i][j] = epi(alpha * sum_k A[b][i][k] * B[b][j][k] + bias[j]) (+ R[b][i][j]) on the fp32 matrix cores
//     (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation in four interleaved k chains added pairwise at
//     the end), 64 x 64 outputs per workgroup, four wavefronts of 32 x 32, K staged through LDS in chunks of 16.  Epilogues: none, ReLU, GELU (erf), tanh.  The
//     strides let the kernel read tokens straight out of NCHW maps (b c h w -> b (h w) c) and write gradients back.
//   * lin_wgrad_kernel + slab_sum_kernel: a Linear layer's weight and bias gradient, dW[o][k] = sum_r dY[r][o] X[r][k].
//     FIXED SPLIT-K: the rows are cut into S slices of L rows (S, L functions of the row count alone), slice s writes
//     its partial sums to ws[s], and a second launch adds the slices in the order s = 0, 1, ..., S-1.
//   * plane LayerNorm (ln_fwd_kernel, ln_bwd_kernel, ln_param_kernel): nn.LayerNorm([H, W]) over (n, c) planes; the
//     parameter gradients by the same fixed split over planes.
//   * DGAB's gate (dgab_pool_*, dgab_gate_*): the H / W means, the concatenation with the point tokens, both softmaxes
//     and the gating, one workgroup per (n, c) plane.
//   * CBAM (cbam_train_fwd_kernel, cbam_bwd_kernel): one workgroup per image; the backward writes per-image parameter
//     gradients as slabs, summed in image order.
// No atomics anywhere: every gradient is bitwise reproducible from run to run and from stream to stream.  No
// allocation and no host synchronisation in the entry points; workspaces come from the caller.
//
// Replaces (reference, mmocr/models/textrecog/): the autograd of backbones/tps_pp/DGAB.py:25-77 and
// backbones/tps_pp/tps_pp.py:27-82,293-323.
#include "tpspp_common.h"
#include "tpspp_dev.h"

#include <math.h>

using namespace tpspp_dev;

namespace {

constexpr int kThreads = 256;
constexpr int TM = 64;          // mm / wgrad: output rows per workgroup
constexpr int TN = 64;          // mm / wgrad: output columns per workgroup
constexpr int TK = 16;          // K chunk staged through LDS
constexpr int kMaxSlices = 512;

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__device__ __forceinline__ float gelu_erf_grad(float x)
{
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143268f;
    return cdf + x * pdf;
}

// ------------------------------------------------------------------------------------------------------------------
// strided batched GEMM
struct MmParams {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    const float* R;
    long long sab, sai, sak, sbb, sbj, sbk, scb, sci, scj;
    int M, N, K, ktot, epi;
    float alpha;
};

__global__ void __launch_bounds__(kThreads)
mm_kernel(const MmParams P)
{
    __shared__ float sA[TK][TM + 1];
    __shared__ float sB[TK][TN + 1];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = tid / kWave;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wv & 1, wn = wv >> 1;
    const long long i0 = (long long)blockIdx.x * TM;
    const int j0 = blockIdx.y * TN;
    const int b = blockIdx.z;
    int Kb = P.K;
    if (P.ktot > 0) {
        const long long rem = (long long)P.ktot - (long long)b * P.K;
        Kb = rem < P.K ? (int)rem : P.K;
    }
    const float* A = P.A + (long long)b * P.sab;
    const float* B = P.B + (long long)b * P.sbb;
    const bool a_kfast = P.sak == 1, b_kfast = P.sbk == 1;

    f32x16 acc4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc4[q][r] = 0.0f;

    for (int k0 = 0; k0 < Kb; k0 += TK) {
#pragma unroll
        for (int r = 0; r < (TM * TK) / kThreads; ++r) {
            const int e = tid + kThreads * r;
            const int kk = a_kfast ? (e & (TK - 1)) : e / TM;
            const int ii = a_kfast ? e / TK : (e & (TM - 1));
            const long long i = i0 + ii;
            const int k = k0 + kk;
            float v = 0.0f;
            if (i < P.M && k < Kb) v = A[i * P.sai + (long long)k * P.sak];
            sA[kk][ii] = v;
        }
#pragma unroll
        for (int r = 0; r < (TN * TK) / kThreads; ++r) {
            const int e = tid + kThreads * r;
            const int kk = b_kfast ? (e & (TK - 1)) : e / TN;
            const int jj = b_kfast ? e / TK : (e & (TN - 1));
            const int j = j0 + jj;
            const int k = k0 + kk;
            float v = 0.0f;
            if (j < P.N && k < Kb) v = B[(long long)j * P.sbj + (long long)k * P.sbk];
            sB[kk][jj] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k2 = 0; k2 < TK; k2 += 2) {
            const float a = sA[k2 + half][wm * 32 + l31];
            const float bv = sB[k2 + half][wn * 32 + l31];
            acc4[(k2 >> 1) & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc4[(k2 >> 1) & 3], 0, 0, 0);
        }
        __syncthreads();
    }
    // four interleaved chains over k (k2 / 2 mod 4), added pairwise: a quarter of the chain length per accumulator
    const f32x16 acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);

    const int j = j0 + wn * 32 + l31;
    if (j >= P.N) return;
    const float bj = P.bias ? P.bias[j] : 0.0f;
    float* C = P.C + (long long)b * P.scb + (long long)j * P.scj;
    const float* R = P.R ? P.R + (long long)b * P.scb + (long long)j * P.scj : nullptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long i = i0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (i >= P.M) continue;
        float v = P.alpha * acc[r];
        if (P.bias) v = v + bj;
        if (P.epi == 1) v = v > 0.0f ? v : 0.0f;
        else if (P.epi == 2) v = gelu_erf(v);
        else if (P.epi == 3) v = tanhf(v);
        if (R) v = R[i * P.sci] + v;
        C[i * P.sci] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Linear weight / bias gradient, fixed split-K over rows
struct WgParams {
    const float* dy;          // (M, O) dense
    const float* x;           // token layout: row r = (b, i), b = r / Mi, i = r % Mi: x[b*xsb + i*xsi + k*xsk]
    float* ws;                // [S][O][K] partial dW, then [S][O] partial db
    long long M, Mi, xsb, xsi, xsk;
    int O, K, L, S;
    int want_dw, want_db;
    int x_act;                // 0: x as stored, 2: GELU(x) (fc2's input recomputed from fc1's pre-activation)
};

__global__ void __launch_bounds__(kThreads)
lin_wgrad_kernel(const WgParams P)
{
    __shared__ float sA[TK][TM + 1];
    __shared__ float sB[TK][TN + 1];
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = tid / kWave;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wv & 1, wn = wv >> 1;
    const int k0t = blockIdx.x * TN;           // input-feature tile
    const int o0 = blockIdx.y * TM;            // output-feature tile
    const int s = blockIdx.z;
    const long long r0 = (long long)s * P.L;
    long long r1 = r0 + P.L;
    if (r1 > P.M) r1 = P.M;
    const bool x_kfast = P.xsk == 1;
    const bool one_batch = P.Mi >= P.M;        // dense rows: no (batch, row) split of r
    const bool do_db = P.want_db && blockIdx.x == 0 && tid < TM;
    float db_acc = 0.0f;                       // bias gradient of column o0 + tid: the staged dy rows, in row order

    f32x16 acc4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc4[q][r] = 0.0f;
    for (long long rc = r0; rc < r1; rc += TK) {
#pragma unroll
        for (int q = 0; q < (TM * TK) / kThreads; ++q) {
            const int e = tid + kThreads * q;
            const int oo = e & (TM - 1), rr = e / TM;
            const long long r = rc + rr;
            const int o = o0 + oo;
            sA[rr][oo] = (r < r1 && o < P.O) ? P.dy[r * P.O + o] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < (TN * TK) / kThreads; ++q) {
            const int e = tid + kThreads * q;
            const int rr = x_kfast ? e / TN : (e & (TK - 1));
            const int kk = x_kfast ? (e & (TN - 1)) : e / TK;
            const long long r = rc + rr;
            const int k = k0t + kk;
            float v = 0.0f;
            if (P.want_dw && r < r1 && k < P.K) {
                long long off;
                if (one_batch) {
                    off = r * P.xsi;
                } else {
                    const unsigned bi = (unsigned)r / (unsigned)P.Mi;      // r < 2^31: checked by the entry point
                    off = (long long)bi * P.xsb + (r - (long long)bi * P.Mi) * P.xsi;
                }
                v = P.x[off + (long long)k * P.xsk];
                if (P.x_act == 2) v = gelu_erf(v);
            }
            sB[rr][kk] = v;
        }
        __syncthreads();
        if (do_db) {
#pragma unroll
            for (int rr = 0; rr < TK; ++rr) db_acc = db_acc + sA[rr][tid];     // rows past r1 were staged as 0
        }
#pragma unroll
        for (int k2 = 0; k2 < TK && P.want_dw; k2 += 2) {
            const float a = sA[k2 + half][wm * 32 + l31];
            const float bv = sB[k2 + half][wn * 32 + l31];
            acc4[(k2 >> 1) & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc4[(k2 >> 1) & 3], 0, 0, 0);
        }
        __syncthreads();
    }
    // four interleaved chains over k (k2 / 2 mod 4), added pairwise: a quarter of the chain length per accumulator
    const f32x16 acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    if (do_db && o0 + tid < P.O) P.ws[(size_t)P.S * P.O * P.K + (size_t)s * P.O + o0 + tid] = db_acc;
    if (!P.want_dw) return;
    const int k = k0t + wn * 32 + l31;
    if (k >= P.K) return;
    float* out = P.ws + (size_t)s * P.O * P.K + k;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (o < P.O) out[(size_t)o * P.K] = acc[r];
    }
}

// out[e] = sum_{s = 0..S-1} ws[s * stride + e], e < E, in that order (the second pass of every fixed split-K here)
__global__ void __launch_bounds__(256)
slab_sum_kernel(const float* __restrict__ ws, int S, long long stride, long long E, float* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || out == nullptr) return;
    float v = 0.0f;
    for (int s = 0; s < S; ++s) v = v + ws[(long long)s * stride + e];
    out[e] = v;
}

struct Split { long long L; int S; };

// rows per slice: at least 256, and at most kMaxSlices slices (a function of the row count alone)
Split split_rows(long long M, long long min_rows)
{
    long long L = (M + kMaxSlices - 1) / kMaxSlices;
    if (L < min_rows) L = min_rows;
    L = (L + TK - 1) / TK * TK;
    Split sp;
    sp.L = L;
    sp.S = (int)((M + L - 1) / L);
    if (sp.S < 1) sp.S = 1;
    return sp;
}

// ------------------------------------------------------------------------------------------------------------------
// pointwise backward of the activations
__global__ void __launch_bounds__(256)
act_bwd_kernel(int op, long long n, const float* __restrict__ g, const float* __restrict__ t, float scale,
               float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gv = g[i], tv = t[i];
    float v;
    if (op == 0) v = tv > 0.0f ? gv : 0.0f;                    // ReLU, t = its output
    else if (op == 1) v = gv * gelu_erf_grad(tv);              // GELU, t = its input
    else v = gv * (1.0f - tv * tv) * scale;                    // tanh(scale * u), t = its output; d/du
    out[i] = v;
}

// ------------------------------------------------------------------------------------------------------------------
// block reduction helper: 256 threads, fixed tree (deterministic)
__device__ __forceinline__ float block_sum(float v, float* red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// LayerNorm over planes of P elements: one workgroup per plane
__global__ void __launch_bounds__(kThreads)
ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int P, float eps,
              float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd)
{
    __shared__ float red[kThreads];
    const long long row = blockIdx.x;
    const float* xr = x + row * P;
    float s = 0.0f;
    for (int p = threadIdx.x; p < P; p += kThreads) s = s + xr[p];
    const float mu = block_sum(s, red) / (float)P;
    float q = 0.0f;
    for (int p = threadIdx.x; p < P; p += kThreads) {
        const float d = xr[p] - mu;
        q = q + d * d;
    }
    const float var = block_sum(q, red) / (float)P;
    const float rs = 1.0f / sqrtf(var + eps);
    if (threadIdx.x == 0) { mean[row] = mu; rstd[row] = rs; }
    float* yr = y + row * P;
    for (int p = threadIdx.x; p < P; p += kThreads) yr[p] = (xr[p] - mu) * rs * w[p] + b[p];
}

__global__ void __launch_bounds__(kThreads)
ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
              const float* __restrict__ mean, const float* __restrict__ rstd, int P, float* __restrict__ dx, int accumulate)
{
    __shared__ float red[kThreads];
    const long long row = blockIdx.x;
    const float* xr = x + row * P;
    const float* gr = dy + row * P;
    const float mu = mean[row], rs = rstd[row];
    float sa = 0.0f, sb = 0.0f;
    for (int p = threadIdx.x; p < P; p += kThreads) {
        const float g = gr[p] * w[p];
        sa = sa + g;
        sb = sb + g * ((xr[p] - mu) * rs);
    }
    const float ma = block_sum(sa, red) / (float)P;
    const float mb = block_sum(sb, red) / (float)P;
    float* dr = dx + row * P;
    for (int p = threadIdx.x; p < P; p += kThreads) {
        const float xh = (xr[p] - mu) * rs;
        const float v = rs * (gr[p] * w[p] - ma - xh * mb);
        dr[p] = accumulate ? dr[p] + v : v;
    }
}

// per slice s: ws[s][p] = sum over its planes of dy * xhat, ws[S + s][p] = sum of dy
__global__ void __launch_bounds__(kThreads)
ln_param_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                const float* __restrict__ rstd, long long rows, int P, long long L, int S, float* __restrict__ ws)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;
    const int s = blockIdx.y;
    if (p >= P) return;
    const long long r0 = (long long)s * L;
    long long r1 = r0 + L;
    if (r1 > rows) r1 = rows;
    float gw = 0.0f, gb = 0.0f;
    for (long long r = r0; r < r1; ++r) {
        const float g = dy[r * P + p];
        gw = gw + g * ((x[r * P + p] - mean[r]) * rstd[r]);
        gb = gb + g;
    }
    ws[(size_t)s * P + p] = gw;
    ws[(size_t)(S + s) * P + p] = gb;
}

// ------------------------------------------------------------------------------------------------------------------
// DGAB gate (DGAB.py:36-44).  Plane (n, c) of xn (H, W); point tokens y in the point map's own layout (N, C, T).
// catw[n][c] = [mean_H xn (W values), y[n][c][:] (T values)], cath[n][c] = [mean_W xn (H values), y[n][c][:]]
__global__ void __launch_bounds__(kThreads)
dgab_pool_fwd_kernel(const float* __restrict__ xn, const float* __restrict__ y, int C, int H, int W, int T,
                     float* __restrict__ catw, float* __restrict__ cath)
{
    const long long pl = blockIdx.x;
    const float* xp = xn + pl * H * W;
    float* cw = catw + pl * (W + T);
    float* ch = cath + pl * (H + T);
    for (int t = threadIdx.x; t < W + H + T; t += kThreads) {
        if (t < W) {
            float s = 0.0f;
            for (int i = 0; i < H; ++i) s = s + xp[i * W + t];
            cw[t] = s / (float)H;
        } else if (t < W + H) {
            const int i = t - W;
            float s = 0.0f;
            for (int j = 0; j < W; ++j) s = s + xp[i * W + j];
            ch[i] = s / (float)W;
        } else {
            const int k = t - W - H;
            const float v = y[pl * T + k];
            cw[W + k] = v;
            ch[H + k] = v;
        }
    }
}

// dxn[n][c][i][j] += dcatw[n][c][j] / H + dcath[n][c][i] / W;  dy[n][c][t] = dcatw[n][c][W + t] + dcath[n][c][H + t]
__global__ void __launch_bounds__(kThreads)
dgab_pool_bwd_kernel(const float* __restrict__ dcatw, const float* __restrict__ dcath, int C, int H, int W, int T,
                     float* __restrict__ dxn, float* __restrict__ dy)
{
    const long long pl = blockIdx.x;
    const float* gw = dcatw + pl * (W + T);
    const float* gh = dcath + pl * (H + T);
    float* dp = dxn + pl * H * W;
    for (int e = threadIdx.x; e < H * W; e += kThreads) {
        const int i = e / W, j = e - i * W;
        dp[e] = dp[e] + (gw[j] / (float)H + gh[i] / (float)W);
    }
    if (dy)
        for (int k = threadIdx.x; k < T; k += kThreads) dy[pl * T + k] = gw[W + k] + gh[H + k];
}

// softmax of v[0..L-1] into out (every thread computes the same max / sum, in the same order)
__device__ __forceinline__ void softmax_lds(const float* v, int L, float* out)
{
    float m = v[0];
    for (int k = 1; k < L; ++k) m = fmaxf(m, v[k]);
    float s = 0.0f;
    for (int k = 0; k < L; ++k) s = s + expf(v[k] - m);
    for (int k = threadIdx.x; k < L; k += kThreads) out[k] = expf(v[k] - m) / s;
}

constexpr int kMaxHW = 4096;
constexpr int kMaxGate = 256;

// A[i][j] = (vh[i] * xn[i][j]) * gh + (vw[j] * xn[i][j]) * gw,  vh = softmax(h[:H]), gh = h[H], vw = softmax(w[:W]), gw = w[W]
__global__ void __launch_bounds__(kThreads)
dgab_gate_fwd_kernel(const float* __restrict__ xn, const float* __restrict__ w, const float* __restrict__ h, int H,
                     int W, float* __restrict__ A)
{
    __shared__ float sw[kMaxGate + 1], sh[kMaxGate + 1], vw[kMaxGate], vh[kMaxGate];
    const long long pl = blockIdx.x;
    for (int k = threadIdx.x; k <= W; k += kThreads) sw[k] = w[pl * (W + 1) + k];
    for (int k = threadIdx.x; k <= H; k += kThreads) sh[k] = h[pl * (H + 1) + k];
    __syncthreads();
    softmax_lds(sw, W, vw);
    softmax_lds(sh, H, vh);
    __syncthreads();
    const float gw = sw[W], gh = sh[H];
    const float* xp = xn + pl * H * W;
    float* ap = A + pl * H * W;
    for (int e = threadIdx.x; e < H * W; e += kThreads) {
        const int i = e / W, j = e - i * W;
        const float x = xp[e];
        ap[e] = vh[i] * x * gh + vw[j] * x * gw;
    }
}

// dxn = dA * (vh[i] gh + vw[j] gw) (overwrites); dw (W + 1), dh (H + 1): gradients of the pre-softmax gate vectors
__global__ void __launch_bounds__(kThreads)
dgab_gate_bwd_kernel(const float* __restrict__ dA, const float* __restrict__ xn, const float* __restrict__ w,
                     const float* __restrict__ h, int H, int W, float* __restrict__ dxn, float* __restrict__ dw,
                     float* __restrict__ dh)
{
    __shared__ float sw[kMaxGate + 1], sh[kMaxGate + 1], vw[kMaxGate], vh[kMaxGate];
    __shared__ float pxy[kMaxHW];
    __shared__ float colsum[kMaxGate], rowsum[kMaxGate];
    __shared__ float dvw[kMaxGate], dvh[kMaxGate];
    const long long pl = blockIdx.x;
    for (int k = threadIdx.x; k <= W; k += kThreads) sw[k] = w[pl * (W + 1) + k];
    for (int k = threadIdx.x; k <= H; k += kThreads) sh[k] = h[pl * (H + 1) + k];
    __syncthreads();
    softmax_lds(sw, W, vw);
    softmax_lds(sh, H, vh);
    __syncthreads();
    const float gw = sw[W], gh = sh[H];
    const float* xp = xn + pl * H * W;
    const float* gp = dA + pl * H * W;
    float* dp = dxn + pl * H * W;
    for (int e = threadIdx.x; e < H * W; e += kThreads) {
        const int i = e / W, j = e - i * W;
        const float g = gp[e];
        pxy[e] = g * xp[e];
        dp[e] = g * vh[i] * gh + g * vw[j] * gw;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += kThreads) {
        float s = 0.0f;
        for (int i = 0; i < H; ++i) s = s + pxy[i * W + j];
        colsum[j] = s;
    }
    for (int i = threadIdx.x; i < H; i += kThreads) {
        float s = 0.0f;
        for (int j = 0; j < W; ++j) s = s + pxy[i * W + j];
        rowsum[i] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < W; j += kThreads) dvw[j] = colsum[j] * gw;
    for (int i = threadIdx.x; i < H; i += kThreads) dvh[i] = rowsum[i] * gh;
    __syncthreads();
    // every thread forms the same dot products (same order), then writes its share
    float dgw = 0.0f, sw_dot = 0.0f;
    for (int j = 0; j < W; ++j) { dgw = dgw + colsum[j] * vw[j]; sw_dot = sw_dot + vw[j] * dvw[j]; }
    float dgh = 0.0f, sh_dot = 0.0f;
    for (int i = 0; i < H; ++i) { dgh = dgh + rowsum[i] * vh[i]; sh_dot = sh_dot + vh[i] * dvh[i]; }
    for (int j = threadIdx.x; j <= W; j += kThreads) dw[pl * (W + 1) + j] = j < W ? vw[j] * (dvw[j] - sw_dot) : dgw;
    for (int i = threadIdx.x; i <= H; i += kThreads) dh[pl * (H + 1) + i] = i < H ? vh[i] * (dvh[i] - sh_dot) : dgh;
}

// ------------------------------------------------------------------------------------------------------------------
// CBAM (tps_pp.py:27-82) on small maps: one workgroup per image, the map in LDS.
constexpr int kCbamMaxC = 256, kCbamMaxCr = 64, kCbamMaxHW = 256, kCbamMaxElems = 4096;

struct CbamParams {
    const float* x;           // (N, C, H, W)
    const float* w1;          // (Cr, C)   shared_MLP[0]
    const float* w2;          // (C, Cr)   shared_MLP[2]
    const float* cw;          // (1, 2, 3, 3) spatial conv
    const float* cb;          // (1)
    float* out;               // forward: (N, C, H, W)
    float* ca;                // (N, C) channel gate
    float* sa;                // (N, H*W) spatial gate
    const float* dout;        // backward
    float* dx;
    float* ws;                // backward: [N][Cr*C + C*Cr + 18 + 1]
    int C, Cr, H, W;
};

// shared front of the forward and the backward: x, out1 = ca * x, channel avg / max (+ argmax), the MLP's hidden layer,
// the spatial map (channel mean / max of out1, + argmax)
struct CbamSmem {
    float x[kCbamMaxElems];
    float o1[kCbamMaxElems];
    float avg[kCbamMaxC], mx[kCbamMaxC], ca[kCbamMaxC];
    int amx[kCbamMaxC];
    float ha[kCbamMaxCr], hm[kCbamMaxCr];
    float sp[2][kCbamMaxHW];
    int asp[kCbamMaxHW];
    float sa[kCbamMaxHW];
};

__device__ void cbam_front(const CbamParams& P, CbamSmem& S, int n)
{
    const int HW = P.H * P.W, CHW = P.C * HW;
    const float* xn = P.x + (long long)n * CHW;
    for (int e = threadIdx.x; e < CHW; e += kThreads) S.x[e] = xn[e];
    __syncthreads();
    for (int c = threadIdx.x; c < P.C; c += kThreads) {
        float s = 0.0f, m = S.x[c * HW];
        int am = 0;
        for (int p = 0; p < HW; ++p) {
            const float v = S.x[c * HW + p];
            s = s + v;
            if (v > m) { m = v; am = p; }
        }
        S.avg[c] = s / (float)HW;
        S.mx[c] = m;
        S.amx[c] = am;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < P.Cr; t += kThreads) {
        float a = 0.0f, m = 0.0f;
        for (int c = 0; c < P.C; ++c) {
            a = a + P.w1[t * P.C + c] * S.avg[c];
            m = m + P.w1[t * P.C + c] * S.mx[c];
        }
        S.ha[t] = a > 0.0f ? a : 0.0f;
        S.hm[t] = m > 0.0f ? m : 0.0f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < P.C; c += kThreads) {
        float za = 0.0f, zm = 0.0f;
        for (int t = 0; t < P.Cr; ++t) {
            za = za + P.w2[c * P.Cr + t] * S.ha[t];
            zm = zm + P.w2[c * P.Cr + t] * S.hm[t];
        }
        S.ca[c] = sigmoidf(za + zm);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CHW; e += kThreads) S.o1[e] = S.ca[e / HW] * S.x[e];
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        float s = 0.0f, m = S.o1[p];
        int am = 0;
        for (int c = 0; c < P.C; ++c) {
            const float v = S.o1[c * HW + p];
            s = s + v;
            if (v > m) { m = v; am = c; }
        }
        S.sp[0][p] = s / (float)P.C;
        S.sp[1][p] = m;
        S.asp[p] = am;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        const int y = p / P.W, x = p - y * P.W;
        float z = 0.0f;
        for (int ch = 0; ch < 2; ++ch)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = y + ky - 1, xx = x + kx - 1;
                    if (yy < 0 || yy >= P.H || xx < 0 || xx >= P.W) continue;
                    z = z + P.cw[(ch * 3 + ky) * 3 + kx] * S.sp[ch][yy * P.W + xx];
                }
        S.sa[p] = sigmoidf(z + P.cb[0]);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kThreads)
cbam_train_fwd_kernel(const CbamParams P)
{
    __shared__ CbamSmem S;
    const int n = blockIdx.x;
    cbam_front(P, S, n);
    const int HW = P.H * P.W, CHW = P.C * HW;
    float* on = P.out + (long long)n * CHW;
    for (int e = threadIdx.x; e < CHW; e += kThreads) on[e] = S.sa[e % HW] * S.o1[e];
    for (int c = threadIdx.x; c < P.C; c += kThreads) P.ca[(long long)n * P.C + c] = S.ca[c];
    for (int p = threadIdx.x; p < HW; p += kThreads) P.sa[(long long)n * HW + p] = S.sa[p];
}

struct CbamBwdSmem {
    float g[kCbamMaxElems];   // d out1
    float dsa[kCbamMaxHW];
    float dsp[2][kCbamMaxHW];
    float dz[kCbamMaxC];
    float dha[kCbamMaxCr], dhm[kCbamMaxCr];
    float davg[kCbamMaxC], dmx[kCbamMaxC];
};

__global__ void __launch_bounds__(kThreads)
cbam_bwd_kernel(const CbamParams P)
{
    __shared__ CbamSmem S;
    __shared__ CbamBwdSmem B;
    const int n = blockIdx.x;
    cbam_front(P, S, n);
    const int HW = P.H * P.W, CHW = P.C * HW;
    const float* gn = P.dout + (long long)n * CHW;
    for (int e = threadIdx.x; e < CHW; e += kThreads) B.g[e] = gn[e] * S.sa[e % HW];
    // d sa, then d z_spatial = d sa * sa (1 - sa)
    for (int p = threadIdx.x; p < HW; p += kThreads) {
        float s = 0.0f;
        for (int c = 0; c < P.C; ++c) s = s + gn[c * HW + p] * S.o1[c * HW + p];
        B.dsa[p] = s * S.sa[p] * (1.0f - S.sa[p]);
    }
    __syncthreads();
    float* wsn = P.ws + (long long)n * (2 * P.C * P.Cr + 19);
    // spatial conv: weight / bias gradient and the gradient of its 2-channel input
    for (int q = threadIdx.x; q < 19; q += kThreads) {
        float s = 0.0f;
        if (q == 18) {
            for (int p = 0; p < HW; ++p) s = s + B.dsa[p];
        } else {
            const int ch = q / 9, ky = (q / 3) % 3, kx = q % 3;
            for (int p = 0; p < HW; ++p) {
                const int y = p / P.W, x = p - y * P.W;
                const int yy = y + ky - 1, xx = x + kx - 1;
                if (yy < 0 || yy >= P.H || xx < 0 || xx >= P.W) continue;
                s = s + B.dsa[p] * S.sp[ch][yy * P.W + xx];
            }
        }
        wsn[2 * P.C * P.Cr + q] = s;
    }
    for (int e = threadIdx.x; e < 2 * HW; e += kThreads) {
        const int ch = e / HW, p = e - ch * HW;
        const int yy = p / P.W, xx = p - yy * P.W;
        float s = 0.0f;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int y = yy - ky + 1, x = xx - kx + 1;
                if (y < 0 || y >= P.H || x < 0 || x >= P.W) continue;
                s = s + P.cw[(ch * 3 + ky) * 3 + kx] * B.dsa[y * P.W + x];
            }
        B.dsp[ch][p] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CHW; e += kThreads) {
        const int c = e / HW, p = e - c * HW;
        float v = B.g[e] + B.dsp[0][p] / (float)P.C;
        if (S.asp[p] == c) v = v + B.dsp[1][p];
        B.g[e] = v;
    }
    __syncthreads();
    // out1 = ca * x
    for (int c = threadIdx.x; c < P.C; c += kThreads) {
        float s = 0.0f;
        for (int p = 0; p < HW; ++p) s = s + B.g[c * HW + p] * S.x[c * HW + p];
        B.dz[c] = s * S.ca[c] * (1.0f - S.ca[c]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < P.C * P.Cr; e += kThreads) {            // dW2[c][t]
        const int c = e / P.Cr, t = e - c * P.Cr;
        wsn[P.Cr * P.C + e] = B.dz[c] * S.ha[t] + B.dz[c] * S.hm[t];
    }
    for (int t = threadIdx.x; t < P.Cr; t += kThreads) {
        float s = 0.0f;
        for (int c = 0; c < P.C; ++c) s = s + P.w2[c * P.Cr + t] * B.dz[c];
        B.dha[t] = S.ha[t] > 0.0f ? s : 0.0f;
        B.dhm[t] = S.hm[t] > 0.0f ? s : 0.0f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < P.Cr * P.C; e += kThreads) {            // dW1[t][c]
        const int t = e / P.C, c = e - t * P.C;
        wsn[e] = B.dha[t] * S.avg[c] + B.dhm[t] * S.mx[c];
    }
    for (int c = threadIdx.x; c < P.C; c += kThreads) {
        float a = 0.0f, m = 0.0f;
        for (int t = 0; t < P.Cr; ++t) {
            a = a + P.w1[t * P.C + c] * B.dha[t];
            m = m + P.w1[t * P.C + c] * B.dhm[t];
        }
        B.davg[c] = a;
        B.dmx[c] = m;
    }
    __syncthreads();
    float* dxn = P.dx + (long long)n * CHW;
    for (int e = threadIdx.x; e < CHW; e += kThreads) {
        const int c = e / HW, p = e - c * HW;
        float v = B.g[e] * S.ca[c] + B.davg[c] / (float)HW;
        if (S.amx[c] == p) v = v + B.dmx[c];
        dxn[e] = v;
    }
}

int launch_slab_sum(const float* ws, int S, long long E, float* out, hipStream_t st, const char* who)
{
    if (out == nullptr || E <= 0) return TPSPP_OK;
    hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, ws, S, E, E, out);
    return tpspp::check_launch(who);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
TPSPP_EXPORT int tpspp_mm_f32(int batch, int M, int N, int K, const float* A, const long long* a_strides, const float* B,
                              const long long* b_strides, float* C, const long long* c_strides, const float* bias,
                              const float* R, int epilogue, float alpha, int k_total, tpspp_stream_t stream)
{
    const char* who = "tpspp_mm_f32";
    TPSPP_REQUIRE(A && B && C && a_strides && b_strides && c_strides, "%s: null pointer", who);
    TPSPP_REQUIRE(batch >= 0 && M >= 0 && N >= 0 && K > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(epilogue >= 0 && epilogue <= 3, "%s: epilogue must be 0 (none), 1 (ReLU), 2 (GELU) or 3 (tanh)", who);
    TPSPP_REQUIRE(batch <= 65535 && (N + TN - 1) / TN <= 65535, "%s: grid too large", who);
    TPSPP_REQUIRE(k_total <= 0 || (long long)k_total <= (long long)batch * K, "%s: k_total exceeds batch * K", who);
    if (batch == 0 || M == 0 || N == 0) return TPSPP_OK;
    MmParams P;
    P.A = A; P.B = B; P.C = C; P.bias = bias; P.R = R;
    P.sab = a_strides[0]; P.sai = a_strides[1]; P.sak = a_strides[2];
    P.sbb = b_strides[0]; P.sbj = b_strides[1]; P.sbk = b_strides[2];
    P.scb = c_strides[0]; P.sci = c_strides[1]; P.scj = c_strides[2];
    P.M = M; P.N = N; P.K = K; P.ktot = k_total; P.epi = epilogue; P.alpha = alpha;
    const dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((N + TN - 1) / TN), (unsigned)batch);
    hipLaunchKernelGGL(mm_kernel, grid, dim3(kThreads), 0, tpspp::as_stream(stream), P);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_linear_bwd_weight_workspace_floats(long long M, int O, int K)
{
    if (M <= 0 || O <= 0 || K <= 0) return 0;
    const Split sp = split_rows(M, 256);
    return (size_t)sp.S * (size_t)O * ((size_t)K + 1);
}

TPSPP_EXPORT int tpspp_linear_bwd_weight(const float* dy, const float* x, const long long* x_layout, int x_act, long long M,
                                         int O, int K, float* dweight, float* dbias, float* ws, size_t ws_floats,
                                         tpspp_stream_t stream)
{
    const char* who = "tpspp_linear_bwd_weight";
    TPSPP_REQUIRE(dy && (dweight || dbias), "%s: null pointer", who);
    TPSPP_REQUIRE(x_act == 0 || x_act == 2, "%s: x_act must be 0 (none) or 2 (GELU)", who);
    TPSPP_REQUIRE(M < (1LL << 31), "%s: more than 2^31 - 1 rows", who);
    TPSPP_REQUIRE(!dweight || (x && x_layout), "%s: null pointer (x)", who);
    TPSPP_REQUIRE(M >= 0 && O > 0 && K > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE((O + TM - 1) / TM <= 65535, "%s: grid too large", who);
    const size_t need = tpspp_linear_bwd_weight_workspace_floats(M, O, K);
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_linear_bwd_weight_workspace_floats(...) = %zu floats, got %zu)",
                  who, need, ws_floats);
    if (M == 0) return TPSPP_OK;
    WgParams P;
    P.dy = dy; P.x = x; P.ws = ws; P.M = M;
    P.Mi = dweight ? x_layout[0] : 1;
    P.xsb = dweight ? x_layout[1] : 0; P.xsi = dweight ? x_layout[2] : 0; P.xsk = dweight ? x_layout[3] : 0;
    TPSPP_REQUIRE(P.Mi > 0, "%s: x_layout[0] (rows per batch entry) must be positive", who);
    P.O = O; P.K = K;
    const Split sp = split_rows(M, 256);
    P.L = (int)sp.L; P.S = sp.S;
    P.want_dw = dweight != nullptr; P.want_db = dbias != nullptr;
    P.x_act = x_act;
    hipStream_t st = tpspp::as_stream(stream);
    const dim3 grid(P.want_dw ? (unsigned)((K + TN - 1) / TN) : 1u, (unsigned)((O + TM - 1) / TM), (unsigned)sp.S);
    hipLaunchKernelGGL(lin_wgrad_kernel, grid, dim3(kThreads), 0, st, P);
    int rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    rc = launch_slab_sum(ws, sp.S, (long long)O * K, dweight, st, who);
    if (rc != TPSPP_OK) return rc;
    return launch_slab_sum(ws + (size_t)sp.S * O * K, sp.S, O, dbias, st, who);
}

TPSPP_EXPORT int tpspp_act_bwd(int op, long long n, const float* grad, const float* t, float scale, float* out,
                               tpspp_stream_t stream)
{
    const char* who = "tpspp_act_bwd";
    TPSPP_REQUIRE(grad && t && out, "%s: null pointer", who);
    TPSPP_REQUIRE(op >= 0 && op <= 2, "%s: op must be 0 (ReLU), 1 (GELU) or 2 (tanh)", who);
    TPSPP_REQUIRE(n >= 0, "%s: bad size", who);
    if (n == 0) return TPSPP_OK;
    hipLaunchKernelGGL(act_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, tpspp::as_stream(stream), op, n,
                       grad, t, scale, out);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_plane_ln_fwd(const float* x, const float* w, const float* b, long long rows, int P, float eps,
                                    float* y, float* mean, float* rstd, tpspp_stream_t stream)
{
    const char* who = "tpspp_plane_ln_fwd";
    TPSPP_REQUIRE(x && w && b && y && mean && rstd, "%s: null pointer", who);
    TPSPP_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL && P > 0, "%s: bad sizes", who);
    if (rows == 0) return TPSPP_OK;
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)rows), dim3(kThreads), 0, tpspp::as_stream(stream), x, w, b, P, eps,
                       y, mean, rstd);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_plane_ln_bwd_workspace_floats(long long rows, int P)
{
    if (rows <= 0 || P <= 0) return 0;
    const Split sp = split_rows(rows, 16);
    return (size_t)sp.S * 2 * (size_t)P;
}

TPSPP_EXPORT int tpspp_plane_ln_bwd(const float* dy, const float* x, const float* w, const float* mean, const float* rstd,
                                    long long rows, int P, float* dx, int accumulate, float* dweight, float* dbias,
                                    float* ws, size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_plane_ln_bwd";
    TPSPP_REQUIRE(dy && x && w && mean && rstd, "%s: null pointer", who);
    TPSPP_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL && P > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1", who);
    const bool params = dweight || dbias;
    const size_t need = params ? tpspp_plane_ln_bwd_workspace_floats(rows, P) : 0;
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_plane_ln_bwd_workspace_floats(...) = %zu floats, got %zu)", who, need,
                  ws_floats);
    if (rows == 0) return TPSPP_OK;
    hipStream_t st = tpspp::as_stream(stream);
    if (dx) {
        hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)rows), dim3(kThreads), 0, st, dy, x, w, mean, rstd, P, dx,
                           accumulate);
        const int rc = tpspp::check_launch(who);
        if (rc != TPSPP_OK) return rc;
    }
    if (!params) return TPSPP_OK;
    const Split sp = split_rows(rows, 16);
    hipLaunchKernelGGL(ln_param_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads), (unsigned)sp.S), dim3(kThreads), 0,
                       st, dy, x, mean, rstd, rows, P, sp.L, sp.S, ws);
    int rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    rc = launch_slab_sum(ws, sp.S, P, dweight, st, who);
    if (rc != TPSPP_OK) return rc;
    return launch_slab_sum(ws + (size_t)sp.S * P, sp.S, P, dbias, st, who);
}

static int dgab_check(const char* who, int N, int C, int H, int W, int T)
{
    TPSPP_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && T >= 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(H <= kMaxGate && W <= kMaxGate && H * W <= kMaxHW, "%s: H, W <= 256 and H * W <= 4096", who);
    TPSPP_REQUIRE((long long)N * C <= 0x7fffffffLL, "%s: too many planes", who);
    return TPSPP_OK;
}

TPSPP_EXPORT int tpspp_dgab_pool_fwd(const float* xn, const float* y, int N, int C, int H, int W, int T, float* catw,
                                     float* cath, tpspp_stream_t stream)
{
    const char* who = "tpspp_dgab_pool_fwd";
    TPSPP_REQUIRE(xn && y && catw && cath, "%s: null pointer", who);
    const int rc = dgab_check(who, N, C, H, W, T);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(dgab_pool_fwd_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, tpspp::as_stream(stream), xn, y,
                       C, H, W, T, catw, cath);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_dgab_pool_bwd(const float* dcatw, const float* dcath, int N, int C, int H, int W, int T,
                                     float* dxn, float* dy, tpspp_stream_t stream)
{
    const char* who = "tpspp_dgab_pool_bwd";
    TPSPP_REQUIRE(dcatw && dcath && dxn, "%s: null pointer", who);
    const int rc = dgab_check(who, N, C, H, W, T);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(dgab_pool_bwd_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, tpspp::as_stream(stream), dcatw,
                       dcath, C, H, W, T, dxn, dy);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_dgab_gate_fwd(const float* xn, const float* w, const float* h, int N, int C, int H, int W, float* A,
                                     tpspp_stream_t stream)
{
    const char* who = "tpspp_dgab_gate_fwd";
    TPSPP_REQUIRE(xn && w && h && A, "%s: null pointer", who);
    const int rc = dgab_check(who, N, C, H, W, 0);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(dgab_gate_fwd_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, tpspp::as_stream(stream), xn, w,
                       h, H, W, A);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_dgab_gate_bwd(const float* dA, const float* xn, const float* w, const float* h, int N, int C, int H,
                                     int W, float* dxn, float* dw, float* dh, tpspp_stream_t stream)
{
    const char* who = "tpspp_dgab_gate_bwd";
    TPSPP_REQUIRE(dA && xn && w && h && dxn && dw && dh, "%s: null pointer", who);
    const int rc = dgab_check(who, N, C, H, W, 0);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    hipLaunchKernelGGL(dgab_gate_bwd_kernel, dim3((unsigned)(N * C)), dim3(kThreads), 0, tpspp::as_stream(stream), dA, xn,
                       w, h, H, W, dxn, dw, dh);
    return tpspp::check_launch(who);
}

static int cbam_check(const char* who, int N, int C, int Cr, int H, int W)
{
    TPSPP_REQUIRE(N >= 0 && N <= 0x7fffffff && C > 0 && Cr > 0 && H > 0 && W > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(C <= kCbamMaxC && Cr <= kCbamMaxCr && H * W <= kCbamMaxHW && C * H * W <= kCbamMaxElems,
                  "%s: C <= 256, C/ratio <= 64, H * W <= 256 and C * H * W <= 4096", who);
    return TPSPP_OK;
}

TPSPP_EXPORT int tpspp_cbam_train_fwd(const float* x, const float* w1, const float* w2, const float* cw, const float* cb,
                                      int N, int C, int Cr, int H, int W, float* out, float* ca, float* sa,
                                      tpspp_stream_t stream)
{
    const char* who = "tpspp_cbam_train_fwd";
    TPSPP_REQUIRE(x && w1 && w2 && cw && cb && out && ca && sa, "%s: null pointer", who);
    const int rc = cbam_check(who, N, C, Cr, H, W);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    CbamParams P = {};
    P.x = x; P.w1 = w1; P.w2 = w2; P.cw = cw; P.cb = cb; P.out = out; P.ca = ca; P.sa = sa;
    P.C = C; P.Cr = Cr; P.H = H; P.W = W;
    hipLaunchKernelGGL(cbam_train_fwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, tpspp::as_stream(stream), P);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_cbam_bwd_workspace_floats(int N, int C, int Cr)
{
    if (N <= 0 || C <= 0 || Cr <= 0) return 0;
    return (size_t)N * (2 * (size_t)C * Cr + 19);
}

TPSPP_EXPORT int tpspp_cbam_bwd(const float* dout, const float* x, const float* w1, const float* w2, const float* cw,
                                const float* cb, int N, int C, int Cr, int H, int W, float* dx, float* dw1, float* dw2,
                                float* dcw, float* dcb, float* ws, size_t ws_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_cbam_bwd";
    TPSPP_REQUIRE(dout && x && w1 && w2 && cw && cb && dx, "%s: null pointer", who);
    const int rc0 = cbam_check(who, N, C, Cr, H, W);
    if (rc0 != TPSPP_OK) return rc0;
    const size_t need = tpspp_cbam_bwd_workspace_floats(N, C, Cr);
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_cbam_bwd_workspace_floats(...) = %zu floats, got %zu)", who, need,
                  ws_floats);
    if (N == 0) return TPSPP_OK;
    CbamParams P = {};
    P.x = x; P.w1 = w1; P.w2 = w2; P.cw = cw; P.cb = cb; P.dout = dout; P.dx = dx; P.ws = ws;
    P.C = C; P.Cr = Cr; P.H = H; P.W = W;
    hipStream_t st = tpspp::as_stream(stream);
    hipLaunchKernelGGL(cbam_bwd_kernel, dim3((unsigned)N), dim3(kThreads), 0, st, P);
    int rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    // the per-image slabs [N][w1 | w2 | conv weight | conv bias], summed in image order
    const long long E = 2LL * C * Cr + 19;
    float* outs[4] = {dw1, dw2, dcw, dcb};
    const long long off[4] = {0, (long long)C * Cr, 2LL * C * Cr, 2LL * C * Cr + 18};
    const long long len[4] = {(long long)C * Cr, (long long)C * Cr, 18, 1};
    for (int q = 0; q < 4; ++q) {
        if (!outs[q]) continue;
        hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)((len[q] + 255) / 256)), dim3(256), 0, st,
                           (const float*)(ws + off[q]), N, E, len[q], outs[q]);
        rc = tpspp::check_launch(who);
        if (rc != TPSPP_OK) return rc;
    }
    return TPSPP_OK;
}
