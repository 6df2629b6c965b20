// The LSTM cell shared by the CRNN recogniser's inference kernel (tpspp_crnn.hip) and its training kernels
// (tpspp_crnn_train.hip): the constants of the work division, the two activations and the body of the recurrence.  The
// body is one template: Save = false is tpspp_crnn_lstm_fwd as it always was, Save = true also stores what the backward
// through time reads.  The two instantiations perform the same operations on h, c and out, in the same order.
#pragma once
#include "tpspp_crnn.h"
#include "tpspp_dev.h"

namespace tpspp_crnn_cell {

using tpspp_dev::kWave;

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

inline bool lstm_group_ok(int g) { return g == 4 || g == 8 || g == 16; }

// blockIdx.x = 2 * block-of-images + direction.  Lane l of a wavefront holds, as the A operand, h[image l & 15][k] and, as
// the B operand, w_hh[unit l & 15][k] for k = 16 b + 4 (l >> 4) + m; its accumulators hold images 4 (l >> 4) + r of unit
// l & 15 -- the same (image, unit) in all four gate tiles, so the cell update needs no exchange and c stays in registers.
// Save: gates (T, N, 2, 4 kHid) gets sigma(a_i), sigma(a_f), tanh(a_g), sigma(a_o) and cell (T, N, 2, kHid) gets c_t.
template <bool Save>
__device__ __forceinline__ void lstm_recurrence(const float* __restrict__ xg, const float* __restrict__ whh,
                                                float* __restrict__ out, float* __restrict__ gates, float* __restrict__ cell,
                                                int T, int N, int g)
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
                if (valid[r]) {
                    const size_t tok = (size_t)t * N + n0 + 4 * quad + r;
                    out[tok * (2 * kHid) + d * kHid + u] = h;
                    if (Save) {
                        float* gt = gates + (tok * 2 + d) * kGates + u;
                        gt[0] = gi;
                        gt[kHid] = gf;
                        gt[2 * kHid] = gg;
                        gt[3 * kHid] = go;
                        cell[(tok * 2 + d) * kHid + u] = c[ut][r];
                    }
                }
            }
        }
        __syncthreads();            // h of this step is complete before any wavefront reads it; the other copy is free
        cur ^= 1;
    }
}

}  // namespace tpspp_crnn_cell
