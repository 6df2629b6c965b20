// CRNNDecoder's training graph on the bf16 matrix cores (include/tpspp.h: tpspp_crnn_lstm_bf16_bwd,
// tpspp_linear_bwd_weight_bf16; the saving forward is an instantiation of tpspp_crnn_dec_bf16.hip's recurrence): the
// backward through time with its product da W_hh on v_mfma_f32_16x16x32_bf16, and the weight gradient of a Linear layer
// whose two operands are both activations, rounded or split while they are staged.
// Replaces (opt-in): the autograd of nn.LSTM's recurrence and input projection in layers/lstm_layer.py:10,14 (reference).
#include "tpspp_common.h"
#include "tpspp_crnn_cell.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;
using namespace tpspp_crnn_cell;

using tpspp::aligned16;

// ---- backward through time -----------------------------------------------------------------------------------------------------
// (the body and its bf16 product: tpspp_crnn_cell.h)
template <bool X3>
__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_bf16_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ gates, const float* __restrict__ cell,
                          const u32x4* __restrict__ wt_all, float* __restrict__ d_xg, int T, int N, int g)
{
    lstm_backward<MulBf16<X3>>(d_out, gates, cell, wt_all, d_xg, nullptr, T, N, g);
}

// ---- the weight gradient -------------------------------------------------------------------------------------------------------
constexpr int kWgThreads = 256;     // 4 wavefronts, 2 x 2, each owns 64 x 64 of the 128 x 128 tile
constexpr int kWgTile = 128;
constexpr int kLdT = 32 + 8;        // LDS stride, in bf16, of one column's 32 rows: 16-byte aligned
constexpr int kWgTarget = 512;      // workgroups aimed at (two per CU)

struct WgArgs {
    const float* DY;
    const float* X;
    float* out;                     // dW, or the workspace when there is more than one slice
    long long sd0, sd1, sd2, sx0, sx1, sx2;
    long long rows;                 // batch * M
    int M, O, K;
    int per;                        // k steps of 32 rows per slice
    int dy_cols, x_cols;            // the operand's column stride is 1: staged along its columns
};

struct WgPlan {
    long long steps;
    int per, slices;
};

WgPlan wg_plan(long long rows, int O, int K)
{
    WgPlan p;
    p.steps = (rows + 31) / 32;
    const long long tiles = (long long)(O / kWgTile) * (K / kWgTile);
    const long long want = tiles >= kWgTarget ? 1 : kWgTarget / (tiles > 0 ? tiles : 1);
    p.per = (int)((p.steps + want - 1) / want);
    if (p.per < 1) p.per = 1;
    p.slices = (int)((p.steps + p.per - 1) / p.per);
    return p;
}

// One operand's 32 rows x 128 columns of a k step, fp32 in registers -> bf16 (hi, lo) in LDS as sT[column][row].
// COLS: thread (column tid & 127, rows 16 (tid >> 7) ..+16); otherwise thread (row tid & 31, columns 16 (tid >> 5) ..+16).
struct WgStage {
    float v[16];

    __device__ __forceinline__ void load(const float* __restrict__ P, long long s0, long long s1, long long s2, int M,
                                         long long rows, long long row0, int col0, bool cols, int tid)
    {
        if (cols) {
            const int c = tid & 127, rg = tid >> 7;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long row = row0 + 16 * rg + k;
                float x = 0.0f;
                if (row < rows) {
                    const long long b = row / M, i = row - b * M;
                    x = P[b * s0 + i * s1 + (long long)(col0 + c) * s2];
                }
                v[k] = x;
            }
        } else {
            const int rr = tid & 31, cg = tid >> 5;
            const long long row = row0 + rr;
            const bool in = row < rows;
            const long long b = in ? row / M : 0, i = in ? row - b * M : 0;
            const float* p = P + b * s0 + i * s1 + (long long)(col0 + 16 * cg) * s2;
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = in ? p[(long long)k * s2] : 0.0f;
        }
    }

    template <bool X3>
    __device__ __forceinline__ void store(unsigned short* sT, bool cols, int tid) const
    {
        constexpr int slab = kWgTile * kLdT;
        if (cols) {
            const int c = tid & 127, rg = tid >> 7;
            u32x4 hi[2], lo[2];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                unsigned h, l;
                split2(v[2 * k], v[2 * k + 1], h, l);
                hi[k >> 2][k & 3] = h;
                lo[k >> 2][k & 3] = l;
            }
            u32x4* ph = reinterpret_cast<u32x4*>(sT + c * kLdT + 16 * rg);
            ph[0] = hi[0];
            ph[1] = hi[1];
            if (X3) {
                u32x4* pl = reinterpret_cast<u32x4*>(sT + slab + c * kLdT + 16 * rg);
                pl[0] = lo[0];
                pl[1] = lo[1];
            }
        } else {
            const int rr = tid & 31, cg = tid >> 5;
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                unsigned h, l;
                split2(v[k], v[k + 1], h, l);
                unsigned short* p = sT + (16 * cg + k) * kLdT + rr;
                p[0] = (unsigned short)h;
                p[kLdT] = (unsigned short)(h >> 16);
                if (X3) {
                    p[slab] = (unsigned short)l;
                    p[slab + kLdT] = (unsigned short)(l >> 16);
                }
            }
        }
    }
};

// blockIdx.x = (slice * O / 128 + i tile) * K / 128 + j tile.  Lane l holds, as the A operand, DY[row 8 (l >> 4) + jj][i = l & 15]
// and, as the B operand, X[row 8 (l >> 4) + jj][j = l & 15] of the k step; its accumulators are dW[i = 4 (l >> 4) + r][j = l & 15].
template <bool X3>
__global__ void __launch_bounds__(kWgThreads)
linear_bwd_weight_bf16_kernel(const WgArgs p)
{
    constexpr int S = X3 ? 2 : 1;
    constexpr int slab = kWgTile * kLdT;
    __shared__ __attribute__((aligned(16))) unsigned short sD[S * slab];
    __shared__ __attribute__((aligned(16))) unsigned short sX[S * slab];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int nj = p.K / kWgTile, ni = p.O / kWgTile;
    const int jt = (int)(blockIdx.x % (unsigned)nj);
    const int it = (int)((blockIdx.x / (unsigned)nj) % (unsigned)ni);
    const int slice = (int)(blockIdx.x / (unsigned)(nj * ni));
    const int wi = wave >> 1, wj = wave & 1;
    const long long step0 = (long long)slice * p.per;
    const long long total = (p.rows + 31) / 32;
    const int nsteps = (int)(total - step0 < p.per ? total - step0 : p.per);

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    WgStage sd, sx;
    const bool dc = p.dy_cols != 0, xc = p.x_cols != 0;
    sd.load(p.DY, p.sd0, p.sd1, p.sd2, p.M, p.rows, step0 * 32, it * kWgTile, dc, tid);
    sx.load(p.X, p.sx0, p.sx1, p.sx2, p.M, p.rows, step0 * 32, jt * kWgTile, xc, tid);
    for (int ks = 0; ks < nsteps; ++ks) {
        __syncthreads();            // the previous k step's fragments are read
        sd.store<X3>(sD, dc, tid);
        sx.store<X3>(sX, xc, tid);
        __syncthreads();
        if (ks + 1 < nsteps) {
            sd.load(p.DY, p.sd0, p.sd1, p.sd2, p.M, p.rows, (step0 + ks + 1) * 32, it * kWgTile, dc, tid);
            sx.load(p.X, p.sx0, p.sx1, p.sx2, p.M, p.rows, (step0 + ks + 1) * 32, jt * kWgTile, xc, tid);
        }
        u32x4 bh[4], bl[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const unsigned short* q = sX + (wj * 64 + nt * 16 + col) * kLdT + 8 * quad;
            bh[nt] = *reinterpret_cast<const u32x4*>(q);
            bl[nt] = X3 ? *reinterpret_cast<const u32x4*>(q + slab) : bh[nt];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const unsigned short* q = sD + (wi * 64 + mt * 16 + col) * kLdT + 8 * quad;
            const u32x4 ah = *reinterpret_cast<const u32x4*>(q);
            u32x4 al = ah;
            if (X3) al = *reinterpret_cast<const u32x4*>(q + slab);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                acc[mt][nt] = mfma_bf16(ah, bh[nt], acc[mt][nt]);           // dy_hi x_hi
                if (X3) {
                    acc[mt][nt] = mfma_bf16(ah, bl[nt], acc[mt][nt]);       // dy_hi x_lo
                    acc[mt][nt] = mfma_bf16(al, bh[nt], acc[mt][nt]);       // dy_lo x_hi
                }
            }
        }
    }
    float* out = p.out + (size_t)slice * p.O * p.K;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = it * kWgTile + wi * 64 + mt * 16 + 4 * quad + r;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) out[(size_t)i * p.K + jt * kWgTile + wj * 64 + nt * 16 + col] = acc[mt][nt][r];
        }
    }
}

// dW = ws[0] + ws[1] + ... in ascending order; slices == 0: all +0.  n4: float4 elements of dW.
__global__ void __launch_bounds__(256)
linear_bwd_weight_bf16_sum_kernel(const f32x4* __restrict__ ws, f32x4* __restrict__ dW, long long n4, int slices)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    f32x4 s = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (slices > 0) s = ws[e];
    for (int k = 1; k < slices; ++k) {
        const f32x4 v = ws[(long long)k * n4 + e];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = s[j] + v[j];
    }
    dW[e] = s;
}

int check_wg(const char* who, int batch, int M, int O, int K)
{
    TPSPP_REQUIRE(batch >= 0 && M >= 0 && O >= 1 && K >= 1, "%s: bad sizes", who);
    TPSPP_REQUIRE(O % kWgTile == 0 && K % kWgTile == 0, "%s: needs O and K multiples of %d, got O %d, K %d", who, kWgTile, O, K);
    TPSPP_REQUIRE((long long)batch * M <= (1LL << 30), "%s: batch * M too large", who);
    TPSPP_REQUIRE((long long)O * K <= (1LL << 30), "%s: O * K too large", who);
    return TPSPP_OK;
}

}  // namespace

TPSPP_EXPORT int tpspp_crnn_lstm_bf16_bwd(const float* d_out, const float* gates, const float* cell, const void* w_hh_t_arranged,
                                          float* d_xg, int T, int N, int hidden, int images_per_group, int split3,
                                          tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_bf16_bwd";
    TPSPP_REQUIRE(d_out && gates && cell && w_hh_t_arranged && d_xg, "%s: null pointer", who);
    TPSPP_REQUIRE(aligned16(w_hh_t_arranged), "%s: w_hh_t_arranged must be 16-byte aligned", who);
    const int rc = check_lstm(who, T, N, hidden, images_per_group, split3);
    if (rc != TPSPP_OK || N == 0) return rc;
    unsigned groups;
    const int g = lstm_grid(N, images_per_group, groups);
    if (g < 0) return g;
    const size_t lds = (split3 ? MulBf16<true>::kBwdLds : MulBf16<false>::kBwdLds) * sizeof(unsigned short);
    static bool attr_done[tpspp::kMaxDevices] = {};
    if (tpspp::first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&crnn_lstm_bf16_bwd_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MulBf16<true>::kBwdLds * sizeof(unsigned short)));
        (void)hipGetLastError();
    }
    const u32x4* w = static_cast<const u32x4*>(w_hh_t_arranged);
    hipStream_t st = tpspp::as_stream(stream);
    if (split3)
        hipLaunchKernelGGL(crnn_lstm_bf16_bwd_kernel<true>, dim3(groups), dim3(kLstmThreads), lds, st, d_out, gates, cell, w, d_xg,
                           T, N, g);
    else
        hipLaunchKernelGGL(crnn_lstm_bf16_bwd_kernel<false>, dim3(groups), dim3(kLstmThreads), lds, st, d_out, gates, cell, w, d_xg,
                           T, N, g);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT size_t tpspp_linear_bwd_weight_bf16_workspace_floats(int batch, int M, int O, int K)
{
    if (batch <= 0 || M <= 0 || O <= 0 || K <= 0 || O % kWgTile || K % kWgTile) return 0;
    const WgPlan pl = wg_plan((long long)batch * M, O, K);
    return pl.slices > 1 ? (size_t)pl.slices * (size_t)O * (size_t)K : 0;
}

TPSPP_EXPORT int tpspp_linear_bwd_weight_bf16(int batch, int M, int O, int K, const float* DY, const long long* dy_strides,
                                              const float* X, const long long* x_strides, float* dW, float* ws, size_t ws_floats,
                                              int split3, tpspp_stream_t stream)
{
    const char* who = "tpspp_linear_bwd_weight_bf16";
    TPSPP_REQUIRE(DY && dy_strides && X && x_strides && dW, "%s: null pointer", who);
    const int rc = check_wg(who, batch, M, O, K);
    if (rc != TPSPP_OK) return rc;
    TPSPP_REQUIRE(split3 == 0 || split3 == 1, "%s: split3 must be 0 or 1, got %d", who, split3);
    for (int i = 0; i < 3; ++i)
        TPSPP_REQUIRE(dy_strides[i] >= 0 && x_strides[i] >= 0, "%s: strides must be >= 0", who);
    TPSPP_REQUIRE(aligned16(dW), "%s: dW must be 16-byte aligned", who);
    const size_t need = tpspp_linear_bwd_weight_bf16_workspace_floats(batch, M, O, K);
    TPSPP_REQUIRE(ws_floats >= need, "%s: workspace of %zu floats, %zu needed", who, ws_floats, need);
    TPSPP_REQUIRE(need == 0 || (ws && aligned16(ws)), "%s: null pointer (ws; 16-byte aligned)", who);
    hipStream_t st = tpspp::as_stream(stream);
    const long long rows = (long long)batch * M;
    const long long n4 = (long long)O * K / 4;
    const unsigned sum_blocks = (unsigned)((n4 + 255) / 256);
    if (rows == 0) {
        hipLaunchKernelGGL(linear_bwd_weight_bf16_sum_kernel, dim3(sum_blocks), dim3(256), 0, st, nullptr,
                           reinterpret_cast<f32x4*>(dW), n4, 0);
        return tpspp::check_launch(who);
    }
    const WgPlan pl = wg_plan(rows, O, K);
    WgArgs p;
    p.DY = DY;
    p.X = X;
    p.out = pl.slices > 1 ? ws : dW;
    p.sd0 = dy_strides[0], p.sd1 = dy_strides[1], p.sd2 = dy_strides[2];
    p.sx0 = x_strides[0], p.sx1 = x_strides[1], p.sx2 = x_strides[2];
    p.rows = rows;
    p.M = M, p.O = O, p.K = K;
    p.per = pl.per;
    p.dy_cols = p.sd2 == 1;
    p.x_cols = p.sx2 == 1;
    const long long blocks = (long long)pl.slices * (O / kWgTile) * (K / kWgTile);
    TPSPP_REQUIRE(blocks < (1LL << 31), "%s: too large", who);
    const dim3 grid((unsigned)blocks), block(kWgThreads);
    if (split3) hipLaunchKernelGGL(linear_bwd_weight_bf16_kernel<true>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(linear_bwd_weight_bf16_kernel<false>, grid, block, 0, st, p);
    int lrc = tpspp::check_launch(who);
    if (lrc != TPSPP_OK || pl.slices == 1) return lrc;
    hipLaunchKernelGGL(linear_bwd_weight_bf16_sum_kernel, dim3(sum_blocks), dim3(256), 0, st, reinterpret_cast<const f32x4*>(ws),
                       reinterpret_cast<f32x4*>(dW), n4, pl.slices);
    return tpspp::check_launch(who);
}
