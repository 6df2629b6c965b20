// Training kernels of the NRTR encoder's and decoder's attention (include/tpspp_train_attn.h, and its generalisation
// tpspp_attn_train_fwd_ex / _bwd_ex of include/tpspp_train_dec.h): scaled-dot-product attention with a key mask
// (valid_ratio prefix, per-key mask, causal) and dropout on the probabilities, forward and backward, exact fp32.
//
// replaces: the autograd of common/modules/transformer_module.py:24-33,71-96 (reference, mmocr/models/) in the
// training graph; tps_pp_amd/ops.py composes it with tpspp_mm_f32 / tpspp_plane_ln_* / tpspp_linear_bwd_weight /
// tpspp_act_bwd into an encoder layer (attn_block_autograd, ffn_block_autograd).
//
// Everything is a 64 x 64 tile (64 = the head width d_k = d_v, one block of queries, one block of keys) and every
// product C[i][j] = sum_k A(i, k) B(j, k) of two such tiles runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation, k ascending in one chain), four wavefronts of 32 x 32 outputs.  A tile is either held in registers as an
// MFMA operand (lane l holds X[row(l & 31)][2t + (l >> 5)], t = 0..31: the tile that stays for the whole workgroup) or
// staged row-major in LDS with a row pitch of 65 words, which both `row` reads (X[idx][k]) and `column` reads (X[k][idx])
// take without bank conflicts.
//   * attn_train_fwd_kernel, one workgroup per (image, head, block of 64 queries), q in registers.  Pass A walks the
//     key blocks and keeps a running row maximum and sum (lse = max + log(sum)); pass B recomputes each S block, forms
//     P = exp(S - lse), applies the dropout and accumulates out += P v.  Key blocks past valid_len, or (causal) wholly
//     above the diagonal of the query block, are never read.
//   * attn_train_bwd_dq_kernel, the same ownership: dS = P * (dropout'(d_out v^T) - rowsum(d_out * out)) per key
//     block, dq += dS k.
//   * attn_train_bwd_dkv_kernel, one workgroup per (image, head, block of 64 keys), k and v in registers: it walks the
//     query blocks and accumulates dv += dropout(P)^T d_out and dk += dS^T q.  (P and dS are computed twice, once per
//     owner: no gradient is shared between workgroups, so there are no atomics and nothing to reduce.)
// Dropout: Philox-4x32-10 keyed by the seed, counter (h << 16 | (i >> 2) << 8 | j, b, offset); its four words decide
// rows 4g .. 4g + 3 of one column -- exactly the four consecutive rows that one accumulator quad of the MFMA layout
// holds, so a lane makes 4 Philox calls for its 16 elements of a block.  Bitwise reproducible: no atomics, fixed orders.
#include "tpspp_common.h"
#include "tpspp_dev.h"
#include "tpspp_train_attn.h"
#include "tpspp_train_dec.h"

#include <math.h>

using namespace tpspp_dev;

namespace {

constexpr int kThreads = 256;
constexpr int BT = 64;            // tile edge: queries per block = keys per block = head width
constexpr int LD = BT + 1;        // LDS row pitch in words
constexpr int kMaxT = 256;
constexpr float kScale = 0.125f;  // 1 / sqrt(64): a power of two, so scaling q or scaling q k^T is the same number

typedef float Tile[BT][LD];

struct AttnParams {
    const float* q;
    const float* k;
    const float* v;
    const float* d_out;
    const float* out_in;      // backward: the forward's out
    const float* lse_in;      // backward: the forward's lse
    float* out;
    float* lse;
    float* dq;
    float* dk;
    float* dv;
    const int* valid_len;
    const unsigned char* key_mask;   // (N, Tk), 0 = masked, or NULL
    long long ld_q, ld_kv, ld_dq, ld_dkv;
    int causal;
    int N, C, heads, Tq, Tk;
    unsigned drop_thr;        // floor(drop_p * 2^32); 0: no dropout
    float inv_keep;           // 1 / (1 - drop_p)
    unsigned seed_lo, seed_hi, off_lo, off_hi;
};

struct U4 {
    unsigned x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// the words that decide rows 4g .. 4g + 3 of column j in (image b, head h): keep iff word >= drop_thr
__device__ __forceinline__ void drop_words(const AttnParams& P, int b, int h, int g, int j, unsigned (&w)[4])
{
    const U4 r = philox4x32_10(U4{((unsigned)h << 16) | ((unsigned)g << 8) | (unsigned)j, (unsigned)b, P.off_lo, P.off_hi},
                               P.seed_lo, P.seed_hi);
    w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
}

// row of accumulator register r within a wavefront's 32 x 32 output (column = lane & 31)
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// rows of a token-major operand as an MFMA register operand: r[t] = X[row][2t + half] (0 for row >= nrows)
__device__ __forceinline__ void load_rows(float (&r)[32], const float* base, long long ld, int row, int nrows, int half)
{
    const float* p = base + (long long)row * ld + half;
#pragma unroll
    for (int t = 0; t < 32; ++t) r[t] = row < nrows ? p[2 * t] : 0.0f;
}

// rows [0, nrows) x 64 columns of a token-major operand into an LDS tile, zeros below
__device__ __forceinline__ void load_tile(Tile& s, const float* base, long long ld, int nrows, int tid)
{
#pragma unroll
    for (int r = 0; r < (BT * BT) / kThreads; ++r) {
        const int e = tid + kThreads * r;
        const int c = e & (BT - 1), row = e >> 6;
        s[row][c] = row < nrows ? base[(long long)row * ld + c] : 0.0f;
    }
}

enum { ROW = 0, COL = 1 };

template <int MODE>
__device__ __forceinline__ float lds_op(const Tile& s, int idx, int k)
{
    return MODE == ROW ? s[idx][k] : s[k][idx];
}

// acc[i][j] += sum_k A(i, k) B(j, k), k = 0..63 ascending; this lane's i / j index is `idx` of the LDS operand(s)
template <int BM>
__device__ __forceinline__ f32x16 mm_reg_lds(const float (&a)[32], const Tile& B, int jn, int half, f32x16 acc)
{
#pragma unroll
    for (int t = 0; t < 32; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], lds_op<BM>(B, jn, 2 * t + half), acc, 0, 0, 0);
    return acc;
}

template <int AM>
__device__ __forceinline__ f32x16 mm_lds_reg(const Tile& A, int im, const float (&b)[32], int half, f32x16 acc)
{
#pragma unroll
    for (int t = 0; t < 32; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_op<AM>(A, im, 2 * t + half), b[t], acc, 0, 0, 0);
    return acc;
}

template <int AM, int BM>
__device__ __forceinline__ f32x16 mm_lds_lds(const Tile& A, int im, const Tile& B, int jn, int half, f32x16 acc)
{
#pragma unroll
    for (int t = 0; t < 32; ++t)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lds_op<AM>(A, im, 2 * t + half), lds_op<BM>(B, jn, 2 * t + half), acc, 0,
                                                   0, 0);
    return acc;
}

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.0f;
    return z;
}

__device__ __forceinline__ int valid_keys(const AttnParams& P, int b)
{
    int vl = P.Tk;
    if (P.valid_len) {
        vl = P.valid_len[b];
        vl = vl < 0 ? 0 : (vl > P.Tk ? P.Tk : vl);
    }
    return vl;
}

// is key j0 + jl of image b (one of the `ncols` keys of its block below valid_len) visible to any query at all
__device__ __forceinline__ bool key_visible(const AttnParams& P, int b, int j0, int jl, int ncols)
{
    return jl < ncols && (!P.key_mask || P.key_mask[(long long)b * P.Tk + j0 + jl] != 0);
}

// the keys a block of queries that ends before row `iend` walks: those below valid_len, causal: and not past its last row
__device__ __forceinline__ int walked_keys(const AttnParams& P, int vl, int iend)
{
    return (P.causal && iend < vl) ? iend : vl;
}

// sD[row] = sum_d a[row][d] * b[row][d] for the 64 rows of a block (0 for row >= nrows): one thread per row, one fmaf
// chain over d ascending from 0 -- the order of the MFMA's own k chain, so that for a row with a single valid key and no
// dropout (out == v) this is bit for bit the d_out . v the kernels form on the matrix cores, and dS is an exact zero as
// in PyTorch's softmax backward.  Both backward kernels call it, so they see the same bits.
__device__ __forceinline__ void row_dots(float* sD, const float* a, const float* b, long long ld, int nrows, int tid)
{
    if (tid >= BT) return;
    float s = 0.0f;
    if (tid < nrows) {
        const float* pa = a + (long long)tid * ld;
        const float* pb = b + (long long)tid * ld;
#pragma unroll 16
        for (int c = 0; c < BT; ++c) s = fmaf(pa[c], pb[c], s);
    }
    sD[tid] = s;
}

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
attn_train_fwd_kernel(const AttnParams P)
{
    __shared__ Tile sK, sV, sS;
    __shared__ float sM[BT], sL[BT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wv & 1, wn = wv >> 1;
    const int nqb = (P.Tq + BT - 1) / BT;
    const int b = blockIdx.x / nqb, i0 = (blockIdx.x % nqb) * BT, h = blockIdx.y;
    const int vl = valid_keys(P, b);
    const int nrows = P.Tq - i0 < BT ? P.Tq - i0 : BT;
    const int kend = walked_keys(P, vl, i0 + nrows);
    const float* kb = P.k + (long long)b * P.Tk * P.ld_kv + h * BT;
    const float* vb = P.v + (long long)b * P.Tk * P.ld_kv + h * BT;
    const int im = wm * 32 + l31, jn = wn * 32 + l31;

    float qr[32];
    load_rows(qr, P.q + ((long long)b * P.Tq + i0) * P.ld_q + h * BT, P.ld_q, im, nrows, half);
    if (tid < BT) {
        sM[tid] = -INFINITY;
        sL[tid] = 0.0f;
    }

    // pass A: running maximum and sum of every row over its visible keys (a masked logit is staged as -inf)
    for (int j0 = 0; j0 < kend; j0 += BT) {
        const int ncols = vl - j0 < BT ? vl - j0 : BT;
        const bool kvis = key_visible(P, b, j0, jn, ncols);
        __syncthreads();
        load_tile(sK, kb + (long long)j0 * P.ld_kv, P.ld_kv, ncols, tid);
        __syncthreads();
        const f32x16 s = mm_reg_lds<ROW>(qr, sK, jn, half, zero16());
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int il = wm * 32 + acc_row(r, half);
            sS[il][jn] = (kvis && (!P.causal || j0 + jn <= i0 + il)) ? kScale * s[r] : -INFINITY;
        }
        __syncthreads();
        const int row = tid >> 2, c0 = (tid & 3) * 16;
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 16; ++c) mx = fmaxf(mx, sS[row][c0 + c]);
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        // a row with no visible key in this block (mx == -inf) keeps its maximum and sum: its terms below are
        // exp(-inf - 0) = 0 and the update is skipped, so -inf - -inf never arises
        const bool any = mx > -INFINITY;
        const float m_old = sM[row];
        const float m_new = any ? fmaxf(m_old, mx) : 0.0f;
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) sum = sum + expf(sS[row][c0 + c] - m_new);
        sum = sum + __shfl_xor(sum, 1);
        sum = sum + __shfl_xor(sum, 2);
        if ((tid & 3) == 0 && any) {
            sL[row] = sL[row] * expf(m_old - m_new) + sum;
            sM[row] = m_new;
        }
    }
    __syncthreads();
    if (tid < BT) {
        const float lse = sM[tid] > -INFINITY ? sM[tid] + logf(sL[tid]) : -INFINITY;     // -inf: no visible key at all
        sM[tid] = lse;
        if (tid < nrows) P.lse[((long long)b * P.heads + h) * P.Tq + i0 + tid] = lse;
    }

    // pass B: P = exp(S - lse), dropout, out += P v
    f32x16 o = zero16();
    for (int j0 = 0; j0 < kend; j0 += BT) {
        const int ncols = vl - j0 < BT ? vl - j0 : BT;
        const bool kvis = key_visible(P, b, j0, jn, ncols);
        __syncthreads();
        load_tile(sK, kb + (long long)j0 * P.ld_kv, P.ld_kv, ncols, tid);
        load_tile(sV, vb + (long long)j0 * P.ld_kv, P.ld_kv, ncols, tid);
        __syncthreads();
        const f32x16 s = mm_reg_lds<ROW>(qr, sK, jn, half, zero16());
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (P.drop_thr) drop_words(P, b, h, (i0 >> 2) + wm * 8 + 2 * g + half, j0 + jn, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const int il = wm * 32 + acc_row(r, half);
                float p = (kvis && (!P.causal || j0 + jn <= i0 + il)) ? expf(kScale * s[r] - sM[il]) : 0.0f;
                if (P.drop_thr) p = w[e] >= P.drop_thr ? p * P.inv_keep : 0.0f;
                sS[il][jn] = p;
            }
        }
        __syncthreads();
        o = mm_lds_lds<ROW, COL>(sS, im, sV, jn, half, o);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, half);
        if (il < nrows) P.out[((long long)b * P.Tq + i0 + il) * P.C + h * BT + jn] = o[r];
    }
}

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
attn_train_bwd_dq_kernel(const AttnParams P)
{
    __shared__ Tile sK, sV, sS;
    __shared__ float sLse[BT], sD[BT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wv & 1, wn = wv >> 1;
    const int nqb = (P.Tq + BT - 1) / BT;
    const int b = blockIdx.x / nqb, i0 = (blockIdx.x % nqb) * BT, h = blockIdx.y;
    const int vl = valid_keys(P, b);
    const int nrows = P.Tq - i0 < BT ? P.Tq - i0 : BT;
    const int kend = walked_keys(P, vl, i0 + nrows);
    const float* kb = P.k + (long long)b * P.Tk * P.ld_kv + h * BT;
    const float* vb = P.v + (long long)b * P.Tk * P.ld_kv + h * BT;
    const long long orow = ((long long)b * P.Tq + i0) * P.C + h * BT;     // d_out and out are dense (N*Tq, C)
    const int im = wm * 32 + l31, jn = wn * 32 + l31;

    float qr[32], gr[32];
    load_rows(qr, P.q + ((long long)b * P.Tq + i0) * P.ld_q + h * BT, P.ld_q, im, nrows, half);
    load_rows(gr, P.d_out + orow, P.C, im, nrows, half);
    row_dots(sD, P.d_out + orow, P.out_in + orow, P.C, nrows, tid);
    if (tid < BT) sLse[tid] = tid < nrows ? P.lse_in[((long long)b * P.heads + h) * P.Tq + i0 + tid] : 0.0f;

    f32x16 dq = zero16();
    for (int j0 = 0; j0 < kend; j0 += BT) {
        const int ncols = vl - j0 < BT ? vl - j0 : BT;
        const bool kvis = key_visible(P, b, j0, jn, ncols);
        __syncthreads();
        load_tile(sK, kb + (long long)j0 * P.ld_kv, P.ld_kv, ncols, tid);
        load_tile(sV, vb + (long long)j0 * P.ld_kv, P.ld_kv, ncols, tid);
        __syncthreads();
        const f32x16 s = mm_reg_lds<ROW>(qr, sK, jn, half, zero16());
        const f32x16 dp = mm_reg_lds<ROW>(gr, sV, jn, half, zero16());
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (P.drop_thr) drop_words(P, b, h, (i0 >> 2) + wm * 8 + 2 * g + half, j0 + jn, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const int il = wm * 32 + acc_row(r, half);
                const bool vis = kvis && il < nrows && (!P.causal || j0 + jn <= i0 + il);
                const float p = vis ? expf(kScale * s[r] - sLse[il]) : 0.0f;
                float d = dp[r];
                if (P.drop_thr) d = w[e] >= P.drop_thr ? d * P.inv_keep : 0.0f;
                sS[il][jn] = p * (d - sD[il]);
            }
        }
        __syncthreads();
        dq = mm_lds_lds<ROW, COL>(sS, im, sK, jn, half, dq);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = wm * 32 + acc_row(r, half);
        if (il < nrows) P.dq[((long long)b * P.Tq + i0 + il) * P.ld_dq + h * BT + jn] = kScale * dq[r];
    }
}

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
attn_train_bwd_dkv_kernel(const AttnParams P)
{
    __shared__ Tile sQ, sG, sS;
    __shared__ float sLse[BT], sD[BT];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wv & 1, wn = wv >> 1;
    const int nkb = (P.Tk + BT - 1) / BT;
    const int b = blockIdx.x / nkb, j0 = (blockIdx.x % nkb) * BT, h = blockIdx.y;
    const int vl = valid_keys(P, b);
    const int nkeys = P.Tk - j0 < BT ? P.Tk - j0 : BT;                       // rows of dk / dv this workgroup owns
    const int ncols = vl - j0 < 0 ? 0 : (vl - j0 < BT ? vl - j0 : BT);       // ... of which valid keys
    const long long grow = ((long long)b * P.Tk + j0) * P.ld_dkv + h * BT;
    const int im = wm * 32 + l31, jn = wn * 32 + l31;

    if (ncols == 0) {                  // a block of masked keys: exact zeros, nothing read
        for (int e = tid; e < nkeys * BT; e += kThreads) {
            const long long o = grow + (long long)(e >> 6) * P.ld_dkv + (e & (BT - 1));
            P.dk[o] = 0.0f;
            P.dv[o] = 0.0f;
        }
        return;
    }

    float kr[32], vr[32];
    load_rows(kr, P.k + ((long long)b * P.Tk + j0) * P.ld_kv + h * BT, P.ld_kv, jn, ncols, half);
    load_rows(vr, P.v + ((long long)b * P.Tk + j0) * P.ld_kv + h * BT, P.ld_kv, jn, ncols, half);
    const bool kvis = key_visible(P, b, j0, jn, ncols);

    // causal: the query blocks before this key block see none of its keys (j0 is a multiple of the block size)
    f32x16 dk = zero16(), dv = zero16();
    for (int i0 = P.causal ? j0 : 0; i0 < P.Tq; i0 += BT) {
        const int nrows = P.Tq - i0 < BT ? P.Tq - i0 : BT;
        const long long orow = ((long long)b * P.Tq + i0) * P.C + h * BT;
        __syncthreads();
        load_tile(sQ, P.q + ((long long)b * P.Tq + i0) * P.ld_q + h * BT, P.ld_q, nrows, tid);
        load_tile(sG, P.d_out + orow, P.C, nrows, tid);
        row_dots(sD, P.d_out + orow, P.out_in + orow, P.C, nrows, tid);
        if (tid < BT) sLse[tid] = tid < nrows ? P.lse_in[((long long)b * P.heads + h) * P.Tq + i0 + tid] : 0.0f;
        __syncthreads();
        const f32x16 s = mm_lds_reg<ROW>(sQ, im, kr, half, zero16());
        const f32x16 dp = mm_lds_reg<ROW>(sG, im, vr, half, zero16());
        f32x16 ds;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            if (P.drop_thr) drop_words(P, b, h, (i0 >> 2) + wm * 8 + 2 * g + half, j0 + jn, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 4 * g + e;
                const int il = wm * 32 + acc_row(r, half);
                const bool vis = kvis && il < nrows && (!P.causal || j0 + jn <= i0 + il);
                const float p = vis ? expf(kScale * s[r] - sLse[il]) : 0.0f;
                float pd = p, d = dp[r];
                if (P.drop_thr) {
                    const bool keep = w[e] >= P.drop_thr;
                    pd = keep ? p * P.inv_keep : 0.0f;
                    d = keep ? d * P.inv_keep : 0.0f;
                }
                ds[r] = p * (d - sD[il]);
                sS[il][jn] = pd;
            }
        }
        __syncthreads();
        dv = mm_lds_lds<COL, COL>(sS, im, sG, jn, half, dv);       // dv[j][d] += sum_i Pd[i][j] d_out[i][d]
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) sS[wm * 32 + acc_row(r, half)][jn] = ds[r];
        __syncthreads();
        dk = mm_lds_lds<COL, COL>(sS, im, sQ, jn, half, dk);       // dk[j][d] += sum_i dS[i][j] q[i][d]
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int jl = wm * 32 + acc_row(r, half);
        if (jl < nkeys) {
            const long long o = grow + (long long)jl * P.ld_dkv + jn;
            const bool seen = key_visible(P, b, j0, jl, ncols);       // a masked key: exact zeros
            P.dk[o] = seen ? kScale * dk[r] : 0.0f;
            P.dv[o] = seen ? dv[r] : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
attn_dropout_mask_kernel(const AttnParams P, unsigned char* mask, long long total)
{
    const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int G = (P.Tq + 3) / 4;
    const int j = (int)(idx % P.Tk);
    long long rest = idx / P.Tk;
    const int g = (int)(rest % G);
    rest /= G;
    const int h = (int)(rest % P.heads), b = (int)(rest / P.heads);
    unsigned w[4];
    drop_words(P, b, h, g, j, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = 4 * g + e;
        if (i < P.Tq) mask[(((long long)b * P.heads + h) * P.Tq + i) * P.Tk + j] = w[e] >= P.drop_thr ? 1 : 0;
    }
}

int check_sizes(const char* who, int N, int heads, int Tq, int Tk, float drop_p)
{
    TPSPP_REQUIRE(N >= 0 && heads > 0 && Tq > 0 && Tk > 0, "%s: bad sizes", who);
    TPSPP_REQUIRE(Tq <= kMaxT && Tk <= kMaxT, "%s: at most %d tokens (got Tq = %d, Tk = %d)", who, kMaxT, Tq, Tk);
    TPSPP_REQUIRE(heads <= 65535, "%s: at most 65535 heads", who);
    TPSPP_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "%s: drop_p must lie in [0, 1)", who);
    TPSPP_REQUIRE((long long)N * ((Tq + BT - 1) / BT) <= 0x7fffffffLL && (long long)N * ((Tk + BT - 1) / BT) <= 0x7fffffffLL,
                  "%s: grid too large", who);
    return TPSPP_OK;
}

int check_operands(const char* who, long long ld_q, long long ld_kv, int C, int heads, int causal)
{
    TPSPP_REQUIRE(C == BT * heads, "%s: C must be 64 * heads (d_k = d_v = 64), got C = %d, heads = %d", who, C, heads);
    TPSPP_REQUIRE(ld_q >= C && ld_kv >= C, "%s: row stride %lld < C = %d", who, ld_q < ld_kv ? ld_q : ld_kv, C);
    TPSPP_REQUIRE(causal == 0 || causal == 1, "%s: causal must be 0 or 1, got %d", who, causal);
    return TPSPP_OK;
}

void set_dropout(AttnParams& P, float drop_p, unsigned long long seed, unsigned long long offset)
{
    const double t = (double)drop_p * 4294967296.0;
    P.drop_thr = (unsigned)(t >= 4294967295.0 ? 4294967295.0 : t);
    P.inv_keep = P.drop_thr ? 1.0f / (1.0f - drop_p) : 1.0f;
    P.seed_lo = (unsigned)seed; P.seed_hi = (unsigned)(seed >> 32);
    P.off_lo = (unsigned)offset; P.off_hi = (unsigned)(offset >> 32);
}

// the one forward and the one backward behind both pairs of entry points: P carries the operands, everything is checked here
int attn_fwd(const char* who, AttnParams& P, float drop_p, unsigned long long seed, unsigned long long offset,
             tpspp_stream_t stream)
{
    TPSPP_REQUIRE(P.q && P.k && P.v && P.out && P.lse, "%s: null pointer", who);
    int rc = check_sizes(who, P.N, P.heads, P.Tq, P.Tk, drop_p);
    if (rc != TPSPP_OK) return rc;
    rc = check_operands(who, P.ld_q, P.ld_kv, P.C, P.heads, P.causal);
    if (rc != TPSPP_OK) return rc;
    if (P.N == 0) return TPSPP_OK;
    set_dropout(P, drop_p, seed, offset);
    const dim3 grid((unsigned)(P.N * ((P.Tq + BT - 1) / BT)), (unsigned)P.heads);
    hipLaunchKernelGGL(attn_train_fwd_kernel, grid, dim3(kThreads), 0, tpspp::as_stream(stream), P);
    return tpspp::check_launch(who);
}

int attn_bwd(const char* who, AttnParams& P, float drop_p, unsigned long long seed, unsigned long long offset,
             tpspp_stream_t stream)
{
    TPSPP_REQUIRE(P.d_out && P.q && P.k && P.v && P.out_in && P.lse_in && P.dq && P.dk && P.dv, "%s: null pointer", who);
    int rc = check_sizes(who, P.N, P.heads, P.Tq, P.Tk, drop_p);
    if (rc != TPSPP_OK) return rc;
    rc = check_operands(who, P.ld_q, P.ld_kv, P.C, P.heads, P.causal);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(P.ld_dq >= P.C && P.ld_dkv >= P.C, "%s: gradient row stride %lld < C = %d", who,
                  P.ld_dq < P.ld_dkv ? P.ld_dq : P.ld_dkv, P.C);
    if (P.N == 0) return TPSPP_OK;
    set_dropout(P, drop_p, seed, offset);
    hipStream_t st = tpspp::as_stream(stream);
    hipLaunchKernelGGL(attn_train_bwd_dq_kernel, dim3((unsigned)(P.N * ((P.Tq + BT - 1) / BT)), (unsigned)P.heads),
                       dim3(kThreads), 0, st, P);
    rc = tpspp::check_launch(who);
    if (rc != TPSPP_OK) return rc;
    hipLaunchKernelGGL(attn_train_bwd_dkv_kernel, dim3((unsigned)(P.N * ((P.Tk + BT - 1) / BT)), (unsigned)P.heads),
                       dim3(kThreads), 0, st, P);
    return tpspp::check_launch(who);
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
TPSPP_EXPORT int tpspp_attn_train_fwd_ex(const float* q, long long ld_q, const float* k, const float* v, long long ld_kv, int N,
                                         int C, int heads, int Tq, int Tk, const int* valid_len,
                                         const unsigned char* key_mask, int causal, float drop_p, unsigned long long seed,
                                         unsigned long long offset, float* out, float* lse, tpspp_stream_t stream)
{
    AttnParams P = {};
    P.q = q; P.k = k; P.v = v; P.out = out; P.lse = lse; P.valid_len = valid_len; P.key_mask = key_mask; P.causal = causal;
    P.ld_q = ld_q; P.ld_kv = ld_kv; P.N = N; P.C = C; P.heads = heads; P.Tq = Tq; P.Tk = Tk;
    return attn_fwd("tpspp_attn_train_fwd_ex", P, drop_p, seed, offset, stream);
}

TPSPP_EXPORT int tpspp_attn_train_bwd_ex(const float* d_out, const float* q, long long ld_q, const float* k, const float* v,
                                         long long ld_kv, const float* out, const float* lse, int N, int C, int heads, int Tq,
                                         int Tk, const int* valid_len, const unsigned char* key_mask, int causal,
                                         float drop_p, unsigned long long seed, unsigned long long offset, float* dq,
                                         long long ld_dq, float* dk, float* dv, long long ld_dkv, tpspp_stream_t stream)
{
    AttnParams P = {};
    P.q = q; P.k = k; P.v = v; P.d_out = d_out; P.out_in = out; P.lse_in = lse; P.valid_len = valid_len;
    P.key_mask = key_mask; P.causal = causal; P.dq = dq; P.dk = dk; P.dv = dv;
    P.ld_q = ld_q; P.ld_kv = ld_kv; P.ld_dq = ld_dq; P.ld_dkv = ld_dkv; P.N = N; P.C = C; P.heads = heads; P.Tq = Tq; P.Tk = Tk;
    return attn_bwd("tpspp_attn_train_bwd_ex", P, drop_p, seed, offset, stream);
}

// the encoder's entry points: a prefix mask alone, one row stride for q, k and v
TPSPP_EXPORT int tpspp_attn_train_fwd(const float* q, const float* k, const float* v, long long ld, int N, int C, int heads,
                                      int Tq, int Tk, const int* valid_len, float drop_p, unsigned long long seed,
                                      unsigned long long offset, float* out, float* lse, tpspp_stream_t stream)
{
    AttnParams P = {};
    P.q = q; P.k = k; P.v = v; P.out = out; P.lse = lse; P.valid_len = valid_len;
    P.ld_q = P.ld_kv = ld; P.N = N; P.C = C; P.heads = heads; P.Tq = Tq; P.Tk = Tk;
    return attn_fwd("tpspp_attn_train_fwd", P, drop_p, seed, offset, stream);
}

TPSPP_EXPORT int tpspp_attn_train_bwd(const float* d_out, const float* q, const float* k, const float* v, long long ld,
                                      const float* out, const float* lse, int N, int C, int heads, int Tq, int Tk,
                                      const int* valid_len, float drop_p, unsigned long long seed,
                                      unsigned long long offset, float* dq, float* dk, float* dv, long long ld_grad,
                                      tpspp_stream_t stream)
{
    AttnParams P = {};
    P.q = q; P.k = k; P.v = v; P.d_out = d_out; P.out_in = out; P.lse_in = lse; P.valid_len = valid_len;
    P.dq = dq; P.dk = dk; P.dv = dv;
    P.ld_q = P.ld_kv = ld; P.ld_dq = P.ld_dkv = ld_grad; P.N = N; P.C = C; P.heads = heads; P.Tq = Tq; P.Tk = Tk;
    return attn_bwd("tpspp_attn_train_bwd", P, drop_p, seed, offset, stream);
}
TPSPP_EXPORT int tpspp_attn_dropout_mask(int N, int heads, int Tq, int Tk, float drop_p, unsigned long long seed,
                                         unsigned long long offset, unsigned char* mask, tpspp_stream_t stream)
{
    const char* who = "tpspp_attn_dropout_mask";
    TPSPP_REQUIRE(mask, "%s: null pointer", who);
    const int rc = check_sizes(who, N, heads, Tq, Tk, drop_p);
    if (rc != TPSPP_OK) return rc;
    if (N == 0) return TPSPP_OK;
    AttnParams P = {};
    P.N = N; P.heads = heads; P.Tq = Tq; P.Tk = Tk;
    set_dropout(P, drop_p, seed, offset);
    const long long total = (long long)N * heads * ((Tq + 3) / 4) * Tk;
    TPSPP_REQUIRE((total + kThreads - 1) / kThreads <= 0x7fffffffLL, "%s: grid too large", who);
    hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       tpspp::as_stream(stream), P, mask, total);
    return tpspp::check_launch(who);
}
