// CRNNDecoder's reduced-precision eval path (include/tpspp.h: tpspp_crnn_lstm_bf16_fwd, tpspp_mm_bf16): the recurrence of a
// bidirectional LSTM layer and its input projection on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16), plain bf16
// operands or the three-term split.  Both read their weight in one arranged layout (ops.arrange_mfma16):
//   [hi | lo][rows / 16][K / 32][64 lanes][8] bf16,  lane l of tile (ct, ks) holds W[16 ct + (l & 15)][32 ks + 8 (l >> 4) + j]
// -- the instruction's B operand as the lane holds it, so a fragment is one 16-byte load and a wavefront's load 1 KB.
// Replaces (opt-in): nn.LSTM's recurrence and input projection in layers/lstm_layer.py:10,14 (reference).
#include "tpspp_common.h"
#include "tpspp_crnn_cell.h"
#include "tpspp_dev.h"

namespace {

using namespace tpspp_dev;
using namespace tpspp_crnn_cell;

using tpspp::aligned16;

// ---- the recurrence ----------------------------------------------------------------------------------------------------------
// (the body and its bf16 product: tpspp_crnn_cell.h.  Save: tpspp_crnn_lstm_bf16_train_fwd)
template <bool X3, bool Save>
__global__ void __launch_bounds__(kLstmThreads)
crnn_lstm_bf16_kernel(const float* __restrict__ xg, const u32x4* __restrict__ whh, float* __restrict__ out,
                      float* __restrict__ gates, float* __restrict__ cell, int T, int N, int g)
{
    lstm_forward<MulBf16<X3>, Save>(xg, whh, out, gates, cell, T, N, g);
}

// ---- the projection ------------------------------------------------------------------------------------------------------------
constexpr int kMmThreads = 256;     // 4 wavefronts, each owns 64 rows x 32 columns of the 64 x 128 tile
constexpr int kMmRows = 64;
constexpr int kMmCols = 128;
constexpr int kLdA = 32 + 8;        // LDS row stride of the A tile in bf16: 16-byte aligned

struct MmArgs {
    const float* A;
    const u32x4* W;
    float* C;
    const float* bias;
    long long sa0, sa1, sa2, sc0, sc1, sc2;
    long long rows;                 // batch * M
    int batch, M, N, K;
    int b_fast;                     // rows are taken in the order (i, b) -- b fastest -- instead of (b, i)
    int a_vec4;                     // k stride 1, A and its other strides 16-byte aligned: rows are read in 16-byte pieces
};

// Row r of the flattened operand -> element offsets of its (b, i) in A and C.
__device__ __forceinline__ void mm_row(const MmArgs& p, long long r, long long& ao, long long& co)
{
    long long b, i;
    if (p.b_fast) { i = r / p.batch; b = r - i * p.batch; }
    else { b = r / p.M; i = r - b * p.M; }
    ao = b * p.sa0 + i * p.sa1;
    co = b * p.sc0 + i * p.sc1;
}

// ALONG_K: the k stride of A is 1 and four neighbouring threads stage the 32 k of one row; otherwise the 64 lanes of a
// wavefront stage 64 consecutive rows of one k (contiguous when the row stride -- or, b_fast, the batch stride -- is 1).
template <bool X3, bool ALONG_K>
__global__ void __launch_bounds__(kMmThreads)
mm_bf16_kernel(const MmArgs p)
{
    constexpr int S = X3 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) unsigned short sA[S][kMmRows * kLdA];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int ncol = p.N / kMmCols, nks = p.K / 32;
    const int ctile = (int)(blockIdx.x % (unsigned)ncol);
    const long long r0 = (long long)(blockIdx.x / (unsigned)ncol) * kMmRows;

    const int srow = ALONG_K ? tid >> 2 : tid & 63;
    const int skq = ALONG_K ? tid & 3 : tid >> 6;
    long long sr = r0 + srow, ao, co;
    if (sr > p.rows - 1) sr = p.rows - 1;           // a row past the end stages the last row again; it is never stored
    mm_row(p, sr, ao, co);
    const float* ap = p.A + ao + (long long)(8 * skq) * p.sa2;
    float v[8];
    auto load = [&](int ks) {
        if (ALONG_K && p.a_vec4) {                  // dense, 16-byte aligned rows: two 16-byte loads
            const f32x4 lo4 = *reinterpret_cast<const f32x4*>(ap + 32 * ks), hi4 = *reinterpret_cast<const f32x4*>(ap + 32 * ks + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lo4[j], v[4 + j] = hi4[j];
            return;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ap[(long long)(32 * ks + j) * p.sa2];
    };
    auto store = [&]() {
        u32x4 hi, lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned h, l;
            split2(v[2 * j], v[2 * j + 1], h, l);
            hi[j] = h;
            lo[j] = l;
        }
        *reinterpret_cast<u32x4*>(&sA[0][srow * kLdA + 8 * skq]) = hi;
        if (X3) *reinterpret_cast<u32x4*>(&sA[S - 1][srow * kLdA + 8 * skq]) = lo;
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const size_t slab = (size_t)(p.N / 16) * nks * kWave;
    const u32x4* w = p.W + ((size_t)(ctile * 8 + wave * 2) * nks) * kWave + lane;

    load(0);
    for (int ks = 0; ks < nks; ++ks) {
        __syncthreads();            // the previous k step's fragments are read
        store();
        __syncthreads();
        if (ks + 1 < nks) load(ks + 1);
        u32x4 bh[2], bl[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            bh[ct] = w[((size_t)ct * nks + ks) * kWave];
            bl[ct] = X3 ? w[slab + ((size_t)ct * nks + ks) * kWave] : bh[ct];
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            const u32x4 ah = *reinterpret_cast<const u32x4*>(&sA[0][(rt * 16 + col) * kLdA + 8 * quad]);
            u32x4 al = ah;
            if (X3) al = *reinterpret_cast<const u32x4*>(&sA[S - 1][(rt * 16 + col) * kLdA + 8 * quad]);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                acc[rt][ct] = mfma_bf16(ah, bh[ct], acc[rt][ct]);           // w_hi a_hi
                if (X3) {
                    acc[rt][ct] = mfma_bf16(al, bh[ct], acc[rt][ct]);       // w_hi a_lo
                    acc[rt][ct] = mfma_bf16(ah, bl[ct], acc[rt][ct]);       // w_lo a_hi
                }
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long row = r0 + rt * 16 + 4 * quad + r;
            if (row >= p.rows) continue;
            mm_row(p, row, ao, co);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int j = ctile * kMmCols + wave * 32 + ct * 16 + col;
                p.C[co + (long long)j * p.sc2] = acc[rt][ct][r] + (p.bias ? p.bias[j] : 0.0f);
            }
        }
    }
}

// the checks after the null pointers, and the launch
template <bool Save>
int launch_lstm_bf16(const char* who, const float* xg, const void* w_hh_arranged, float* out, float* gates, float* cell, int T,
                     int N, int hidden, int images_per_group, int split3, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(aligned16(w_hh_arranged), "%s: w_hh_arranged must be 16-byte aligned", who);
    const int rc = check_lstm(who, T, N, hidden, images_per_group, split3);
    if (rc != TPSPP_OK || N == 0) return rc;
    unsigned groups;
    const int g = lstm_grid(N, images_per_group, groups);
    if (g < 0) return g;
    const u32x4* w = static_cast<const u32x4*>(w_hh_arranged);
    if (split3)
        hipLaunchKernelGGL((crnn_lstm_bf16_kernel<true, Save>), dim3(groups), dim3(kLstmThreads), 0, tpspp::as_stream(stream), xg,
                           w, out, gates, cell, T, N, g);
    else
        hipLaunchKernelGGL((crnn_lstm_bf16_kernel<false, Save>), dim3(groups), dim3(kLstmThreads), 0, tpspp::as_stream(stream), xg,
                           w, out, gates, cell, T, N, g);
    return tpspp::check_launch(who);
}

}  // namespace

TPSPP_EXPORT int tpspp_crnn_lstm_bf16_fwd(const float* xg, const void* w_hh_arranged, float* out, int T, int N, int hidden,
                                          int images_per_group, int split3, tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_bf16_fwd";
    TPSPP_REQUIRE(xg && w_hh_arranged && out, "%s: null pointer", who);
    return launch_lstm_bf16<false>(who, xg, w_hh_arranged, out, nullptr, nullptr, T, N, hidden, images_per_group, split3, stream);
}

TPSPP_EXPORT int tpspp_crnn_lstm_bf16_train_fwd(const float* xg, const void* w_hh_arranged, float* out, float* gates,
                                                float* cell, int T, int N, int hidden, int images_per_group, int split3,
                                                tpspp_stream_t stream)
{
    const char* who = "tpspp_crnn_lstm_bf16_train_fwd";
    TPSPP_REQUIRE(xg && w_hh_arranged && out && gates && cell, "%s: null pointer", who);
    return launch_lstm_bf16<true>(who, xg, w_hh_arranged, out, gates, cell, T, N, hidden, images_per_group, split3, stream);
}

TPSPP_EXPORT int tpspp_mm_bf16(int batch, int M, int N, int K, const float* A, const long long* a_strides,
                               const void* B_arranged, float* C, const long long* c_strides, const float* bias, int split3,
                               tpspp_stream_t stream)
{
    const char* who = "tpspp_mm_bf16";
    TPSPP_REQUIRE(A && a_strides && B_arranged && C && c_strides, "%s: null pointer", who);
    TPSPP_REQUIRE(aligned16(B_arranged), "%s: B_arranged must be 16-byte aligned", who);
    TPSPP_REQUIRE(batch >= 0 && M >= 0 && N >= 0 && K >= 1, "%s: bad sizes", who);
    TPSPP_REQUIRE(K % 32 == 0 && N % kMmCols == 0, "%s: needs K a multiple of 32 and N a multiple of %d, got K %d, N %d", who,
                  kMmCols, K, N);
    TPSPP_REQUIRE(split3 == 0 || split3 == 1, "%s: split3 must be 0 or 1, got %d", who, split3);
    for (int i = 0; i < 3; ++i)
        TPSPP_REQUIRE(a_strides[i] >= 0 && c_strides[i] >= 0, "%s: strides must be >= 0", who);
    const long long rows = (long long)batch * M;
    TPSPP_REQUIRE(rows <= (1LL << 30), "%s: batch * M too large", who);
    if (rows == 0 || N == 0) return TPSPP_OK;
    const long long blocks = (rows + kMmRows - 1) / kMmRows * (N / kMmCols);
    TPSPP_REQUIRE(blocks < (1LL << 31), "%s: too large", who);
    MmArgs p;
    p.A = A;
    p.W = static_cast<const u32x4*>(B_arranged);
    p.C = C;
    p.bias = bias;
    p.sa0 = a_strides[0], p.sa1 = a_strides[1], p.sa2 = a_strides[2];
    p.sc0 = c_strides[0], p.sc1 = c_strides[1], p.sc2 = c_strides[2];
    p.rows = rows;
    p.batch = batch, p.M = M, p.N = N, p.K = K;
    const bool along_k = p.sa2 == 1;
    p.b_fast = !along_k && p.sa1 != 1 && p.sa0 == 1;
    p.a_vec4 = along_k && aligned16(A) && p.sa0 % 4 == 0 && p.sa1 % 4 == 0;
    const dim3 grid((unsigned)blocks), block(kMmThreads);
    hipStream_t st = tpspp::as_stream(stream);
    if (split3) {
        if (along_k) hipLaunchKernelGGL((mm_bf16_kernel<true, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((mm_bf16_kernel<true, false>), grid, block, 0, st, p);
    } else {
        if (along_k) hipLaunchKernelGGL((mm_bf16_kernel<false, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((mm_bf16_kernel<false, false>), grid, block, 0, st, p);
    }
    return tpspp::check_launch(who);
}
