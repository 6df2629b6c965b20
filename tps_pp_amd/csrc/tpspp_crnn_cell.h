// The LSTM recurrence of the CRNN recogniser, once per direction of time: lstm_forward<P, Save> is the body of
// tpspp_crnn.hip's crnn_lstm_kernel, tpspp_crnn_train.hip's crnn_lstm_train_kernel and tpspp_crnn_dec_bf16.hip's
// crnn_lstm_bf16_kernel<X3, Save>; lstm_backward<P> is the body of crnn_lstm_bwd_kernel (tpspp_crnn_train.hip) and of
// crnn_lstm_bf16_bwd_kernel<X3> (tpspp_crnn_dec_bf16_train.hip).  A skeleton holds the work division, the valid rows, the
// loads and stores of the saved state, the cell update or the gate-gradient arithmetic, and the barriers; the product policy
// P -- MulF32 on v_mfma_f32_16x16x4f32, MulBf16<X3> on v_mfma_f32_16x16x32_bf16 -- holds how h or da is kept in LDS and how it
// is multiplied by w_hh.  So every instantiation performs the same operations on h, c, out, gates, cell and d_xg in the same
// order, whatever the product and whether or not it saves.  The host side of the entry points shares check_lstm and lstm_grid.
#pragma once
#include "tpspp_crnn.h"
#include "tpspp_common.h"
#include "tpspp_dev.h"

namespace tpspp_crnn_cell {

using tpspp_dev::f32x4;
using tpspp_dev::kWave;
using tpspp_dev::u32x4;

constexpr int kHid = TPSPP_CRNN_HIDDEN;     // units per direction
constexpr int kGates = 4 * kHid;            // gate columns per direction: i, f, g, o
constexpr int kRows = 16;                   // image rows of the matrix-core tile
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

// ---- the host side of the six entry points -----------------------------------------------------------------------------------
inline bool lstm_group_ok(int g) { return g == 4 || g == 8 || g == 16; }

// (split3: the bf16 entry points' switch; the fp32 ones have none)
inline int check_lstm(const char* who, int T, int N, int hidden, int images_per_group, int split3 = 0)
{
    TPSPP_REQUIRE(hidden == kHid, "%s: hidden must be %d, got %d", who, kHid, hidden);
    TPSPP_REQUIRE(T >= 1 && N >= 0, "%s: bad sizes (T >= 1, N >= 0)", who);
    TPSPP_REQUIRE(images_per_group == 0 || lstm_group_ok(images_per_group), "%s: images_per_group must be 0, 4, 8 or 16, got %d",
                  who, images_per_group);
    TPSPP_REQUIRE(split3 == 0 || split3 == 1, "%s: split3 must be 0 or 1, got %d", who, split3);
    TPSPP_REQUIRE((long long)T * N <= (1LL << 30), "%s: T * N too large", who);
    return TPSPP_OK;
}

// N > 0 -> the images per workgroup g of tpspp_crnn_lstm_plan (< 0: its error) and the grid, 2 directions x ceil(N / g) blocks
inline int lstm_grid(int N, int images_per_group, unsigned& groups)
{
    const int g = tpspp_crnn_lstm_plan(N, images_per_group, 0);
    groups = g > 0 ? 2u * (unsigned)((N + g - 1) / g) : 0u;
    return g;
}

// ---- the product policies ------------------------------------------------------------------------------------------------------
// Forward: kFwdLds elements of Lds hold one copy of h (the skeleton keeps two); store_h writes h of (image row, unit u) into the
// copy of the next step, fwd_product adds h W_hh^T of the 16 units of `tile`, all four gates, to acc.  (It is handed the tile's
// index and the lane's unit u = 16 tile + col, and each policy uses only the one its addresses are made of: where the fp32
// product derives u from the tile index itself, that index has two users and the compiler no longer derives the second tile's
// three global addresses as constant offsets of the first's -- 6 to 8 VGPRs, and a wave of occupancy in the saving kernel.)
// Backward: kBwdLds elements hold da; stage writes the four gate gradients of (image row, unit u), bwd_product gives
// dhr = da W_hh of the wavefront's two tiles.
// fwd_weights / bwd_weights: the lane's view of direction d's w_hh / its transpose.

// Exact fp32.  Forward: lane l holds, as the A operand, h[image l & 15][k] and, as the B operand, w_hh[unit l & 15][k] for
// k = 16 b + 4 (l >> 4) + m.  Backward: as the A operand da[image l & 15][j], as the B operand w_hh_t[unit l & 15][j],
// j = 16 b + 4 (l >> 4) + m.
struct MulF32 {
    typedef float Lds;
    typedef float Weight;
    static constexpr int kLd = kHid + 4;            // LDS row stride of h in floats: 16-byte aligned, rows 4 banks apart
    static constexpr int kDaLd = kGates + 4;        // LDS row stride of da in floats: rows 4 banks apart
    static constexpr int kFwdLds = kRows * kLd;
    static constexpr int kBwdLds = kRows * kDaLd;   // 65792 bytes

    static __device__ __forceinline__ const float* fwd_weights(const float* whh, int d, int) { return whh + (size_t)d * kGates * kHid; }

    static __device__ __forceinline__ void store_h(float* hn, int row, int u, float h) { hn[row * kLd + u] = h; }

    static __device__ __forceinline__ void fwd_product(const float* hcur, const float* w, int, int u, int col, int quad, f32x4 (&acc)[4])
    {
        const float* hrow = hcur + col * kLd + 4 * quad;
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
    }

    static __device__ __forceinline__ const float* bwd_weights(const float* wt_all, int d, int) { return wt_all + (size_t)d * kHid * kGates; }

    static __device__ __forceinline__ void stage(float* da, int row, int u, const float (&a)[4])
    {
#pragma unroll
        for (int q = 0; q < 4; ++q) da[row * kDaLd + q * kHid + u] = a[q];
    }

    static __device__ __forceinline__ void bwd_product(const float* da, const float* wt, int wave, int col, int quad, float (&dhr)[2][4])
    {
        f32x4 acc[2][2];
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) acc[ut][0] = acc[ut][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float* arow = da + col * kDaLd + 4 * quad;
        const float* w0 = wt + (size_t)((2 * wave) * 16 + col) * kGates + 4 * quad;
        const float* w1 = w0 + (size_t)16 * kGates;
#pragma unroll 2
        for (int b = 0; b < kGates / 16; b += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {                           // two accumulation chains per tile: even b, odd b
                const f32x4 av = *reinterpret_cast<const f32x4*>(arow + 16 * (b + h));
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(w0 + 16 * (b + h));
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(w1 + 16 * (b + h));
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    acc[0][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], b0[m], acc[0][h], 0, 0, 0);
                    acc[1][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], b1[m], acc[1][h], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dhr[ut][r] = acc[ut][0][r] + acc[ut][1][r];
        }
    }
};

// The bf16 matrix cores, plain bf16 operands or (X3) the three-term split: h and da are rounded or split as they are stored,
// the hi copy first, the lo copy one slab behind it; the weight is ops.arrange_mfma16's layout (tpspp_crnn_dec_bf16.hip), a
// fragment one 16-byte load.  Forward: lane l holds, as the A operand, h[image l & 15][k = 32 b + 8 (l >> 4) + j].  Backward:
// as the A operand da[image l & 15][j = 32 b + 8 (l >> 4) + jj], as the B operand w_hh[d][j][unit] from the arranged transpose.
template <bool X3>
struct MulBf16 {
    typedef unsigned short Lds;
    typedef u32x4 Weight;
    static constexpr int S = X3 ? 2 : 1;
    static constexpr int kLdH = kHid + 8;           // LDS row stride of h in bf16: 16-byte aligned, rows 4 banks apart
    static constexpr int kLdDa = kGates + 8;        // LDS row stride of da in bf16: 16-byte aligned, rows 4 banks apart
    static constexpr int kHSlab = kRows * kLdH;     // bf16 elements of one (hi or lo) copy of h
    static constexpr int kDaSlab = kRows * kLdDa;   // ... of da
    static constexpr int kFwdLds = S * kHSlab;
    static constexpr int kBwdLds = S * kDaSlab;     // 66048 bytes with the split
    static constexpr int kWhhSlab = (kGates / 16) * (kHid / 32) * kWave;    // 16-byte units of one direction's w_hh slab
    static constexpr int kWtSlab = (kHid / 16) * (kGates / 32) * kWave;     // ... of its arranged transpose

    static __device__ __forceinline__ const u32x4* fwd_weights(const u32x4* whh, int d, int lane) { return whh + (size_t)d * S * kWhhSlab + lane; }

    static __device__ __forceinline__ void store_h(unsigned short* hn, int row, int u, float h)
    {
        unsigned hi, lo;
        tpspp_dev::split2(h, 0.0f, hi, lo);
        hn[row * kLdH + u] = (unsigned short)hi;
        if (X3) hn[kHSlab + row * kLdH + u] = (unsigned short)lo;
    }

    static __device__ __forceinline__ void fwd_product(const unsigned short* hcur, const u32x4* w, int tile, int, int col, int quad, f32x4 (&acc)[4])
    {
        using tpspp_dev::mfma_bf16;
        const unsigned short* hrow = hcur + col * kLdH + 8 * quad;
        // (unrolled by two only: all eight steps' weight fragments in flight at once spill)
#pragma unroll 2
        for (int b = 0; b < kHid / 32; ++b) {
            const u32x4 ah = *reinterpret_cast<const u32x4*>(hrow + 32 * b);
            u32x4 al = ah;
            if (X3) al = *reinterpret_cast<const u32x4*>(hrow + kHSlab + 32 * b);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4* wt = w + ((q * 16 + tile) * (kHid / 32) + b) * kWave;
                const u32x4 bh = wt[0];
                acc[q] = mfma_bf16(ah, bh, acc[q]);                     // w_hi h_hi
                if (X3) {
                    acc[q] = mfma_bf16(al, bh, acc[q]);                 // w_hi h_lo
                    acc[q] = mfma_bf16(ah, wt[kWhhSlab], acc[q]);       // w_lo h_hi
                }
            }
        }
    }

    static __device__ __forceinline__ const u32x4* bwd_weights(const u32x4* wt_all, int d, int lane) { return wt_all + (size_t)d * S * kWtSlab + lane; }

    static __device__ __forceinline__ void stage(unsigned short* da, int row, int u, const float (&a)[4])
    {
        unsigned short* dn = &da[row * kLdDa + u];
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            unsigned hi, lo;
            tpspp_dev::split2(a[q], a[q + 1], hi, lo);
            dn[q * kHid] = (unsigned short)hi;
            dn[(q + 1) * kHid] = (unsigned short)(hi >> 16);
            if (X3) {
                dn[kDaSlab + q * kHid] = (unsigned short)lo;
                dn[kDaSlab + (q + 1) * kHid] = (unsigned short)(lo >> 16);
            }
        }
    }

    static __device__ __forceinline__ void bwd_product(const unsigned short* da, const u32x4* wt, int wave, int col, int quad, float (&dhr)[2][4])
    {
        using tpspp_dev::mfma_bf16;
        f32x4 acc[2];
        acc[0] = acc[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const unsigned short* arow = da + col * kLdDa + 8 * quad;
        const u32x4* w0 = wt + (size_t)(2 * wave) * (kGates / 32) * kWave;
#pragma unroll 4
        for (int b = 0; b < kGates / 32; ++b) {
            const u32x4 ah = *reinterpret_cast<const u32x4*>(arow + 32 * b);
            u32x4 al = ah;
            if (X3) al = *reinterpret_cast<const u32x4*>(arow + kDaSlab + 32 * b);
#pragma unroll
            for (int ut = 0; ut < 2; ++ut) {
                const u32x4* wf = w0 + ((size_t)ut * (kGates / 32) + b) * kWave;
                const u32x4 bh = wf[0];
                acc[ut] = mfma_bf16(ah, bh, acc[ut]);               // w_hi da_hi
                if (X3) {
                    acc[ut] = mfma_bf16(al, bh, acc[ut]);           // w_hi da_lo
                    acc[ut] = mfma_bf16(ah, wf[kWtSlab], acc[ut]);  // w_lo da_hi
                }
            }
        }
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dhr[ut][r] = acc[ut][r];
        }
    }
};

// ---- forward in time -----------------------------------------------------------------------------------------------------------
// blockIdx.x = 2 * block-of-images + direction; wavefront w owns the units 32 w .. 32 w + 31.  A lane's accumulators hold images
// 4 (l >> 4) + r of unit l & 15 of a tile -- the same (image, unit) in all four gate tiles, so the cell update needs no exchange
// and c stays in registers.
// Save: gates (T, N, 2, 4 kHid) gets sigma(a_i), sigma(a_f), tanh(a_g), sigma(a_o) and cell (T, N, 2, kHid) gets c_t.
template <class P, bool Save>
__device__ __forceinline__ void lstm_forward(const float* __restrict__ xg, const typename P::Weight* __restrict__ whh,
                                             float* __restrict__ out, float* __restrict__ gates, float* __restrict__ cell, int T,
                                             int N, int g)
{
    __shared__ __attribute__((aligned(16))) typename P::Lds hbuf[2][P::kFwdLds];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int d = blockIdx.x & 1;
    const int n0 = (int)(blockIdx.x >> 1) * g;
    const int col = lane & 15, quad = lane >> 4;
    for (int i = tid; i < 2 * P::kFwdLds; i += kLstmThreads) (&hbuf[0][0])[i] = 0;
    const typename P::Weight* w = P::fwd_weights(whh, d, lane);
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
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int tile = 2 * wave + ut;
            const int u = tile * 16 + col;
            f32x4 acc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* x = xg + (((size_t)t * N + (valid[r] ? n0 + 4 * quad + r : 0)) * 2 + d) * kGates + u;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q][r] = valid[r] ? x[q * kHid] : 0.0f;
            }
            P::fwd_product(hbuf[cur], w, tile, u, col, quad, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gi = sigmoid_safe(acc[0][r]), gf = sigmoid_safe(acc[1][r]);
                const float gg = tanh_safe(acc[2][r]), go = sigmoid_safe(acc[3][r]);
                c[ut][r] = gf * c[ut][r] + gi * gg;
                const float h = go * tanh_safe(c[ut][r]);
                P::store_h(hbuf[cur ^ 1], 4 * quad + r, u, h);      // rows past the block: xg = 0 keeps c = h = 0
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

// ---- backward through time -----------------------------------------------------------------------------------------------------
// The forward's division and lane <-> (image, unit) map; the accumulators of da W_hh are dh_rec of the lane's own (image, unit)
// pairs, so neither dc nor dh_rec leaves the registers.  d_xg gets the unrounded fp32 da; d_xg_dir, where not null, its
// direction-major copy (2, T, N, 4 kHid).  Dynamic LDS: P::kBwdLds elements.
template <class P>
__device__ __forceinline__ void lstm_backward(const float* __restrict__ d_out, const float* __restrict__ gates,
                                              const float* __restrict__ cell, const typename P::Weight* __restrict__ wt_all,
                                              float* __restrict__ d_xg, float* __restrict__ d_xg_dir, int T, int N, int g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lstm_bwd_lds[];
    typename P::Lds* da = reinterpret_cast<typename P::Lds*>(lstm_bwd_lds);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int d = blockIdx.x & 1;
    const int n0 = (int)(blockIdx.x >> 1) * g;
    const int col = lane & 15, quad = lane >> 4;
    const typename P::Weight* wt = P::bwd_weights(wt_all, d, lane);
    float dc[2][4], dhr[2][4], cc[2][4];
    bool valid[4];
    const int tfirst = d ? 0 : T - 1;                               // the step the forward visited last
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        valid[r] = 4 * quad + r < g && n0 + 4 * quad + r < N;
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int u = (2 * wave + ut) * 16 + col;
            dc[ut][r] = dhr[ut][r] = 0.0f;
            cc[ut][r] = valid[r] ? cell[(((size_t)tfirst * N + n0 + 4 * quad + r) * 2 + d) * kHid + u] : 0.0f;
        }
    }
    for (int s = 0; s < T; ++s) {
        const int t = d ? s : T - 1 - s;
        const bool more = s + 1 < T;                                // a step before this one in the forward's order
        const int tp = d ? t + 1 : t - 1;
#pragma unroll
        for (int ut = 0; ut < 2; ++ut) {
            const int u = (2 * wave + ut) * 16 + col;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                float cprev = 0.0f;
                if (valid[r]) {
                    const size_t n = (size_t)(n0 + 4 * quad + r);
                    const size_t tok = (size_t)t * N + n;
                    const float* gt = gates + (tok * 2 + d) * kGates + u;
                    const float gi = gt[0], gf = gt[kHid], gg = gt[2 * kHid], go = gt[3 * kHid];
                    if (more) cprev = cell[(((size_t)tp * N + n) * 2 + d) * kHid + u];
                    const float dh = d_out[tok * (2 * kHid) + d * kHid + u] + dhr[ut][r];
                    const float tc = tanh_safe(cc[ut][r]);
                    const float dgo = dh * tc;
                    const float dcv = dc[ut][r] + dh * go * (1.0f - tc * tc);
                    a[0] = dcv * gg * gi * (1.0f - gi) + 0.0f;      // + 0.0f: a zero gradient is +0, whatever the signs
                    a[1] = dcv * cprev * gf * (1.0f - gf) + 0.0f;
                    a[2] = dcv * gi * (1.0f - gg * gg) + 0.0f;
                    a[3] = dgo * go * (1.0f - go) + 0.0f;
                    dc[ut][r] = dcv * gf;
                    float* dx = d_xg + (tok * 2 + d) * kGates + u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) dx[q * kHid] = a[q];
                    if (d_xg_dir) {                                 // the direction-major copy: dense rows for d w_hh
                        float* dd = d_xg_dir + ((size_t)d * T * N + tok) * kGates + u;
#pragma unroll
                        for (int q = 0; q < 4; ++q) dd[q * kHid] = a[q];
                    }
                }
                cc[ut][r] = cprev;
                if (more) P::stage(da, 4 * quad + r, u, a);         // rows past the block: 0
            }
        }
        if (!more) break;                                           // nothing reads dh_rec after the last step
        __syncthreads();                                            // da of this step is complete
        P::bwd_product(da, wt, wave, col, quad, dhr);
        __syncthreads();                                            // every wavefront has read da: the next step may write it
    }
}

}  // namespace tpspp_crnn_cell
