// Backward of the fused fp32 convolution of tpspp_conv.hip (res_mode 0, no post-affine):
//     Y = act(conv(cat_c(up(src_0), up(src_1), up(src_2)), W) + b),   act = none | ReLU,
// 1x1 or 3x3 kernel with "same" padding, stride (sh, sw) in {1,2}^2, integer nearest-upsample factors per source.
// Everything runs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ordered fp32 accumulation),
// in the C/D layout the forward kernel uses (col = lane&31 = 32 consecutive pixels / weight columns, row =
// (reg&3) + 8*(reg>>2) + 4*(lane>>5)).  dZ = dY * [Y > 0] (PyTorch's threshold_backward on the in-place ReLU's output)
// is formed as dY is staged into LDS: no dZ tensor reaches HBM.
//
// Data gradient (conv_bwd_data_kernel, one launch per source that wants a gradient):
//     dsrc[n][c][y][x] = sum_{a<uh, b<uw} sum_{co, ky, kx} W[co][c_off + c][ky][kx] * dZ[n][co][oy][ox],
//     (oy, ox) = ((y*uh + a + ph - ky) / sh, (x*uw + b + pw - kx) / sw) when divisible and inside the output.
// GEMM view D[c][pixel] = W^T[c][k] * G[k][pixel], k = (tap, co): the weight is the A operand (read in PyTorch's
// (Cout, Cin, KH, KW) layout, nothing rearranged), the gathered dZ the B operand.  Workgroup = 128 source pixels x 64
// source channels, 4 wavefronts of 32 pixels x 64 channels, like the forward kernel.
//   * stride 2 (on a source that is not upsampled along that axis): the sub-pixel split -- the source pixels are
//     grouped by parity (blockIdx.z carries the class), and a class only iterates over the taps of its parity
//     (3x3: 1 or 2 of 3 per axis), so no MFMA multiplies a tap that can never be valid.  A class without taps (1x1,
//     stride 2, odd rows / columns) has an empty K loop and stores exact zeros: no memset.
//   * nearest upsampling: the uh x uw footprint is folded into the B operand as it is staged (the gathered dZ of
//     the footprint are summed before the MFMA), so the epilogue stores the source's gradient directly; no
//     logical-size gradient and no reduction kernel.  The footprint sum changes the order of the terms only.
//
// Weight / bias gradient (conv_bwd_weight_kernel + conv_bwd_reduce_kernel):
//     dW[co][ci][ky][kx] = sum_{n, oy, ox} dZ[n][co][oy][ox] * X[n][ci][oy*sh - ph + ky][ox*sw - pw + kx]
//     db[co]             = sum_{n, oy, ox} dZ[n][co][oy][ox]
// X the logical (upsampled, concatenated) input, read straight from the sources.  GEMM view D[co][kf] = dZ[co][r] *
// Xcol[r][kf], kf = (ci, ky, kx) (PyTorch's order, so D is dW's layout), reduction over r = (n, oy, ox).  Workgroup =
// 64 output channels x 128 kf; the reduction runs in chunks of 32 pixels.  FIXED SPLIT-K: the N*Ho*Wo terms are cut
// into S slices (S a function of the shapes alone); slice s writes its partial sums to ws[s] and a second launch adds
// the slices in the order s = 0, 1, ..., S-1.  No atomics anywhere: dW and db are bitwise reproducible from run to
// run and from stream to stream (MIOpen's backward-weights solvers do not promise that).
//
// Replaces (reference, mmocr/models/textrecog/): the autograd of mmcv ConvModule / nn.Conv2d (+ nn.Upsample, torch.cat)
// at backbones/tps_pp/tps_pp.py:126-131,149-169,537-562.
// Bound: MFMA for the large layers; the gathers of the staging pass for the small ones.
#include "tpspp_common.h"
#include "tpspp_dev.h"

using namespace tpspp_dev;

namespace {

constexpr int kThreads = 256;
constexpr int BP = 128;        // data gradient: source pixels per workgroup
constexpr int BC = 64;         // data gradient: source channels per workgroup
constexpr int BK = 128;        // weight gradient: kf = (ci, ky, kx) columns per workgroup
constexpr int BO = 64;         // weight gradient: output channels per workgroup
constexpr int RP = 32;         // weight gradient: reduction pixels per chunk
constexpr int kTargetWgs = 1024;  // split-K: slices so that a layer fills ~4 workgroups per CU of a 256-CU part
constexpr int kMaxSlices = 512;

struct BwdSrc {
    const float* p;
    int C, H, W;              // stored size
    int uh, uw;               // nearest upsampling factors
};

__device__ __forceinline__ float masked_dz(const float* dy, const float* y, size_t o)
{
    const float g = dy[o];
    if (y == nullptr) return g;
    return y[o] > 0.0f ? g : 0.0f;
}

// ------------------------------------------------------------------------------------------------------------------
// data gradient
struct BwdDataParams {
    const float* dy;          // (N, Cout, Ho, Wo)
    const float* y;           // (N, Cout, Ho, Wo) when act = ReLU, else null
    const float* w;           // (Cout, Cin, KH, KW)
    float* dx;                // (N, C, H, W): this source's gradient
    int N, Cout, Cin, Ho, Wo, sh, sw, ph, pw;
    int c_off;                // first channel of this source in the concatenation
    int C, H, W, uh, uw;
    int cy, cx;               // parity classes along y / x (2: sub-pixel split, 1: every tap, checked per pixel)
};

template <int KH>
__global__ void __launch_bounds__(kThreads, 2)
conv_bwd_data_kernel(const BwdDataParams P)
{
    constexpr int KW = KH;
    constexpr int KC = KH == 1 ? 32 : 8;           // output channels per K chunk
    constexpr int KCK = KC * KH * KW;              // k values per chunk, at most
    __shared__ float sG[KCK][BP];                  // gathered dZ, k-major
    __shared__ float sA[KCK][BC + 1];              // weights, k-major (+1: conflict-free transposed stores)

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = tid / kWave;
    const int ncls = P.cy * P.cx;
    const int n = blockIdx.z / ncls;
    const int cls = blockIdx.z - n * ncls;
    const int qy = cls / P.cx, qx = cls - qy * P.cx;
    // pixels of this class: y = qy + cy*j, x = qx + cx*i
    const int Hc = (P.H - qy + P.cy - 1) / P.cy, Wc = (P.W - qx + P.cx - 1) / P.cx;
    const int npix = Hc * Wc;
    const int m0 = blockIdx.x * BP;
    if (m0 >= npix) return;                        // uniform over the workgroup (classes differ in size by a row)
    const int c_base = blockIdx.y * BC;

    // taps of the class: ky = ky0 + ksy * j (j < nky); with the sub-pixel split only the taps of the class's parity
    const int ky0 = P.cy == 2 ? (qy + P.ph) & 1 : 0, ksy = P.cy;
    const int kx0 = P.cx == 2 ? (qx + P.pw) & 1 : 0, ksx = P.cx;
    const int nky = (KH - ky0 + ksy - 1) / ksy, nkx = (KW - kx0 + ksx - 1) / ksx;
    const int ntaps = nky * nkx;
    const int kck = KC * ntaps;                    // even: KC is

    // this thread's pixel for the staging pass
    const int sm = tid & (BP - 1);
    const int skk0 = tid >> 7;                     // 0 or 1
    const int spix = m0 + sm;
    const bool spix_ok = spix < npix;
    const int sj = spix_ok ? spix / Wc : 0;
    const int sy = qy + P.cy * sj, sx = qx + P.cx * (spix_ok ? spix - sj * Wc : 0);
    const size_t HoWo = (size_t)P.Ho * P.Wo;
    const float* dyn = P.dy + (size_t)n * P.Cout * HoWo;
    const float* yn = P.y ? P.y + (size_t)n * P.Cout * HoWo : nullptr;

    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    const int half = lane >> 5, l31 = lane & 31;
    const int TAPS = KH * KW;

    // k is ordered (tap, channel-in-chunk): k = t * KC + col.  A thread stages pixel sm for the channels col = skk0,
    // skk0 + 2, ... of every tap; the output position a tap reads is found once per tap and chunk, then KC / 2 loads
    // of consecutive output channels follow (no division in the loop)
    constexpr int NCOL = KC / 2;
    for (int co0 = 0; co0 < P.Cout && kck > 0; co0 += KC) {
        // ---- B: sG[t*KC + col][m] = sum over the footprint of dZ[co0 + col][output position of tap t] ----
        for (int t = 0, jy = 0, jx = 0; t < ntaps; ++t) {
            const int ky = ky0 + ksy * jy, kx = kx0 + ksx * jx;
            float v[NCOL];
#pragma unroll
            for (int i = 0; i < NCOL; ++i) v[i] = 0.0f;
            if (spix_ok) {
                for (int a = 0; a < P.uh; ++a) {
                    const int oyn = sy * P.uh + a + P.ph - ky;
                    if (oyn < 0 || (oyn & (P.sh - 1))) continue;
                    const int oy = oyn >> (P.sh - 1);
                    if (oy >= P.Ho) continue;
                    for (int b = 0; b < P.uw; ++b) {
                        const int oxn = sx * P.uw + b + P.pw - kx;
                        if (oxn < 0 || (oxn & (P.sw - 1))) continue;
                        const int ox = oxn >> (P.sw - 1);
                        if (ox >= P.Wo) continue;
                        const size_t off = (size_t)(co0 + skk0) * HoWo + (size_t)oy * P.Wo + ox;
#pragma unroll
                        for (int i = 0; i < NCOL; ++i) {
                            if (co0 + skk0 + 2 * i < P.Cout)
                                v[i] = v[i] + masked_dz(dyn, yn, off + (size_t)(2 * i) * HoWo);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NCOL; ++i) sG[t * KC + skk0 + 2 * i][sm] = v[i];
            if (++jx == nkx) { jx = 0; ++jy; }
        }
        // ---- A: sA[t*KC + col][c] = W[co0 + col][c_off + c_base + c][tap t] ----
        for (int t = 0, jy = 0, jx = 0; t < ntaps; ++t) {
            const int tap = (ky0 + ksy * jy) * KW + kx0 + ksx * jx;
#pragma unroll
            for (int e = tid; e < KC * BC; e += kThreads) {
                const int col = e / BC, c = e - col * BC;     // BC: a power of two
                const int co = co0 + col;
                float v = 0.0f;
                if (co < P.Cout && c_base + c < P.C)
                    v = P.w[((size_t)co * P.Cin + P.c_off + c_base + c) * TAPS + tap];
                sA[t * KC + col][c] = v;
            }
            if (++jx == nkx) { jx = 0; ++jy; }
        }
        __syncthreads();
        for (int k2 = 0; k2 < kck; k2 += 2) {
            const float b = sG[k2 + half][wv * 32 + l31];
            const float a0 = sA[k2 + half][l31];
            const float a1 = sA[k2 + half][32 + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
        __syncthreads();
    }

    const int pix = m0 + wv * 32 + l31;
    if (pix < npix) {
        const int j = pix / Wc;
        const int y = qy + P.cy * j, x = qx + P.cx * (pix - j * Wc);
        float* out = P.dx + (size_t)n * P.C * P.H * P.W + (size_t)y * P.W + x;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = c_base + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (c < P.C) out[(size_t)c * P.H * P.W] = h2 ? acc1[r] : acc0[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// weight / bias gradient
struct BwdWeightParams {
    BwdSrc src[3];
    int nsrc;
    const float* dy;
    const float* y;
    float* ws;                // [S][Cout][Kf] partial dW, then [S][Cout] partial db
    int N, Cin, Cout, Hi, Wi, Ho, Wo, sh, sw, ph, pw;
    int Kf;                   // Cin * KH * KW
    long long R;              // N * Ho * Wo
    int chunks_per_slice, S;
    int want_dw, want_db;     // want_dw = 0: bias gradient only (one kf tile per slice, no GEMM)
};

template <int KH>
__global__ void __launch_bounds__(kThreads, 2)
conv_bwd_weight_kernel(const BwdWeightParams P)
{
    constexpr int KW = KH, TAPS = KH * KW;
    __shared__ float sZ[RP][BO + 1];               // masked dY, pixel-major (+1: conflict-free transposed stores)
    __shared__ float sX[RP][BK + 1];               // im2col rows of the chunk's pixels

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = tid / kWave;
    const int kf_base = blockIdx.x * BK;
    const int co_base = blockIdx.y * BO;
    const int s = blockIdx.z;
    const long long HoWo = (long long)P.Ho * P.Wo;
    const long long r_begin = (long long)s * P.chunks_per_slice * RP;
    const long long r_end = min(P.R, r_begin + (long long)P.chunks_per_slice * RP);
    const int p = tid & (RP - 1);                  // staging: this thread's pixel of the chunk
    const int g = tid >> 5;                        // ... and its group of rows (8 groups)
    const bool do_db = P.want_db && blockIdx.x == 0;
    const bool do_dw = P.want_dw != 0;

    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
    float dbacc = 0.0f;
    const int half = lane >> 5, l31 = lane & 31;

    for (long long r0 = r_begin; r0 < r_end; r0 += RP) {
        const long long r = r0 + p;
        const bool ok = r < r_end;
        int n = 0, oy = 0, ox = 0;
        long long rem = 0;
        if (ok) {
            n = (int)(r / HoWo);
            rem = r - (long long)n * HoWo;
            oy = (int)(rem / P.Wo);
            ox = (int)(rem - (long long)oy * P.Wo);
        }
        // ---- sZ[p][co] = dZ[n][co_base + co][oy][ox] ----
#pragma unroll
        for (int j = 0; j < BO / 8; ++j) {
            const int co = g + 8 * j;
            float v = 0.0f;
            if (ok && co_base + co < P.Cout)
                v = masked_dz(P.dy, P.y, ((size_t)n * P.Cout + co_base + co) * HoWo + rem);
            sZ[p][co] = v;
        }
        // ---- sX[p][kf] = X[n][ci][oy*sh - ph + ky][ox*sw - pw + kx] (0 outside) ----
        const int iy0 = oy * P.sh - P.ph, ix0 = ox * P.sw - P.pw;
#pragma unroll 4
        for (int j = 0; j < (do_dw ? BK / 8 : 0); ++j) {
            const int kf = g + 8 * j;
            const int kg = kf_base + kf;
            float v = 0.0f;
            if (ok && kg < P.Kf) {
                const int ci = kg / TAPS, t = kg - ci * TAPS;
                const int ky = t / KW, kx = t - ky * KW;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < P.Hi && ix >= 0 && ix < P.Wi) {
                    int c = ci;
                    BwdSrc sc = P.src[0];
                    if (P.nsrc > 1 && c >= sc.C) {
                        c -= sc.C;
                        sc = P.src[1];
                        if (P.nsrc > 2 && c >= sc.C) { c -= sc.C; sc = P.src[2]; }
                    }
                    const int yy = sc.uh == 1 ? iy : iy / sc.uh;
                    const int xx = sc.uw == 1 ? ix : ix / sc.uw;
                    v = sc.p[(((size_t)n * sc.C + c) * sc.H + yy) * sc.W + xx];
                }
            }
            sX[p][kf] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int k2 = 0; k2 < (do_dw ? RP : 0); k2 += 2) {
            const float b = sX[k2 + half][wv * 32 + l31];
            const float a0 = sZ[k2 + half][l31];
            const float a1 = sZ[k2 + half][32 + l31];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
        if (do_db && tid < BO) {                   // fixed order: pixel by pixel
            for (int q = 0; q < RP; ++q) dbacc = dbacc + sZ[q][tid];
        }
        __syncthreads();
    }

    const size_t CK = (size_t)P.Cout * P.Kf;
    const int kf = kf_base + wv * 32 + l31;
    if (do_dw && kf < P.Kf) {
        float* out = P.ws + (size_t)s * CK + kf;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co_base + 32 * h2 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (co < P.Cout) out[(size_t)co * P.Kf] = h2 ? acc1[r] : acc0[r];
            }
        }
    }
    if (do_db && tid < BO && co_base + tid < P.Cout)
        P.ws[(size_t)P.S * CK + (size_t)s * P.Cout + co_base + tid] = dbacc;
}

// dW[i] = sum_s ws[s][i], db[co] = sum_s ws_db[s][co]: the slices in a fixed order
__global__ void __launch_bounds__(256)
conv_bwd_reduce_kernel(const float* __restrict__ ws, int S, long long CK, int Cout, float* __restrict__ dw,
                       float* __restrict__ db)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < CK) {
        if (dw == nullptr) return;
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v = v + ws[(size_t)s * CK + i];
        dw[i] = v;
    } else if (i < CK + Cout) {
        if (db == nullptr) return;
        const int co = (int)(i - CK);
        const float* p = ws + (size_t)S * CK;
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v = v + p[(size_t)s * Cout + co];
        db[co] = v;
    }
}

// split-K geometry: a function of the shapes only (the slices, and with them the result's bits, never depend on the
// device or the stream)
struct SplitK { int chunks_per_slice, S; };

SplitK split_k(long long R, int Cout, int Kf)
{
    const long long chunks = (R + RP - 1) / RP;
    const long long tiles = (long long)((Kf + BK - 1) / BK) * ((Cout + BO - 1) / BO);
    long long S = (kTargetWgs + tiles - 1) / tiles;
    S = S < 1 ? 1 : (S > kMaxSlices ? kMaxSlices : S);
    if (S > chunks) S = chunks;
    if (S < 1) S = 1;
    const long long per = (chunks + S - 1) / S;
    SplitK k;
    k.chunks_per_slice = (int)per;
    k.S = (int)((chunks + per - 1) / per);
    return k;
}

// common argument checks of the two backward entry points; fills the logical input size and the total channel count
int check_common(const char* who, const int* src_dims, int nsrc, int N, int Cout, int KH, int KW, int sh, int sw,
                 int Ho, int Wo, int* Hi_out, int* Wi_out, int* Cin_out)
{
    TPSPP_REQUIRE(src_dims, "%s: null pointer (src_dims)", who);
    TPSPP_REQUIRE(nsrc >= 1 && nsrc <= 3, "%s: 1..3 sources", who);
    TPSPP_REQUIRE((KH == 1 && KW == 1) || (KH == 3 && KW == 3), "%s: kernel must be 1x1 or 3x3", who);
    TPSPP_REQUIRE((sh == 1 || sh == 2) && (sw == 1 || sw == 2), "%s: stride must be 1 or 2 along each axis", who);
    TPSPP_REQUIRE(N >= 0 && Cout > 0 && Ho > 0 && Wo > 0, "%s: bad sizes", who);
    int Hi = -1, Wi = -1, cin = 0;
    for (int i = 0; i < nsrc; ++i) {
        const int* d = src_dims + 5 * i;
        TPSPP_REQUIRE(d[0] > 0 && d[1] > 0 && d[2] > 0 && d[3] >= 1 && d[4] >= 1, "%s: bad source %d", who, i);
        const int lh = d[1] * d[3], lw = d[2] * d[4];
        TPSPP_REQUIRE(Hi < 0 || (Hi == lh && Wi == lw), "%s: sources disagree on the logical size", who);
        Hi = lh; Wi = lw;
        cin += d[0];
    }
    const int ph = (KH - 1) / 2, pw = (KW - 1) / 2;
    TPSPP_REQUIRE(Ho == (Hi + 2 * ph - KH) / sh + 1 && Wo == (Wi + 2 * pw - KW) / sw + 1,
                  "%s: output size does not match input size / stride ('same' padding)", who);
    *Hi_out = Hi; *Wi_out = Wi; *Cin_out = cin;
    return TPSPP_OK;
}

}  // namespace

TPSPP_EXPORT int tpspp_conv2d_bwd_data(float* const* dsrc_ptrs, const int* src_dims, int nsrc, const float* weight,
                                       const float* dy, const float* y, int relu, int N, int Cout, int KH, int KW,
                                       int sh, int sw, int Ho, int Wo, tpspp_stream_t stream)
{
    const char* who = "tpspp_conv2d_bwd_data";
    TPSPP_REQUIRE(dsrc_ptrs && weight && dy, "%s: null pointer", who);
    TPSPP_REQUIRE(relu == 0 || relu == 1, "%s: activation code must be 0 (none) or 1 (ReLU)", who);
    TPSPP_REQUIRE(relu == 0 || y, "%s: null pointer (y is needed for the ReLU mask)", who);
    int Hi, Wi, Cin;
    const int rc = check_common(who, src_dims, nsrc, N, Cout, KH, KW, sh, sw, Ho, Wo, &Hi, &Wi, &Cin);
    if (rc != TPSPP_OK) return rc;
    bool any = false;
    for (int i = 0; i < nsrc; ++i) any = any || dsrc_ptrs[i] != nullptr;
    TPSPP_REQUIRE(any, "%s: null pointer (no source gradient requested)", who);
    TPSPP_REQUIRE((Cout + 0LL) * Cin * KH * KW < (1LL << 31), "%s: weight too large", who);
    if (N == 0) return TPSPP_OK;
    hipStream_t st = tpspp::as_stream(stream);
    int c_off = 0;
    for (int i = 0; i < nsrc; ++i) {
        const int* d = src_dims + 5 * i;
        BwdDataParams P;
        P.dy = dy; P.y = relu ? y : nullptr; P.w = weight; P.dx = dsrc_ptrs[i];
        P.N = N; P.Cout = Cout; P.Cin = Cin; P.Ho = Ho; P.Wo = Wo; P.sh = sh; P.sw = sw;
        P.ph = (KH - 1) / 2; P.pw = (KW - 1) / 2;
        P.c_off = c_off;
        P.C = d[0]; P.H = d[1]; P.W = d[2]; P.uh = d[3]; P.uw = d[4];
        P.cy = (sh == 2 && P.uh == 1) ? 2 : 1;
        P.cx = (sw == 2 && P.uw == 1) ? 2 : 1;
        c_off += d[0];
        if (P.dx == nullptr) continue;
        const int Hc = (P.H + P.cy - 1) / P.cy, Wc = (P.W + P.cx - 1) / P.cx;
        const long long gz = (long long)N * P.cy * P.cx;
        TPSPP_REQUIRE(gz <= 65535 && (P.C + BC - 1) / BC <= 65535, "%s: grid too large", who);
        const dim3 grid((unsigned)((Hc * Wc + BP - 1) / BP), (unsigned)((P.C + BC - 1) / BC), (unsigned)gz);
        if (KH == 1) hipLaunchKernelGGL(conv_bwd_data_kernel<1>, grid, dim3(kThreads), 0, st, P);
        else         hipLaunchKernelGGL(conv_bwd_data_kernel<3>, grid, dim3(kThreads), 0, st, P);
        const int lr = tpspp::check_launch(who);
        if (lr != TPSPP_OK) return lr;
    }
    return TPSPP_OK;
}

TPSPP_EXPORT size_t tpspp_conv2d_bwd_weight_workspace_floats(const int* src_dims, int nsrc, int N, int Cout, int KH,
                                                             int KW, int Ho, int Wo)
{
    if (!src_dims || nsrc < 1 || nsrc > 3 || N <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || Ho <= 0 || Wo <= 0) return 0;
    long long cin = 0;
    for (int i = 0; i < nsrc; ++i) cin += src_dims[5 * i] > 0 ? src_dims[5 * i] : 0;
    const int Kf = (int)(cin * KH * KW);
    const SplitK k = split_k((long long)N * Ho * Wo, Cout, Kf);
    return (size_t)k.S * (size_t)Cout * ((size_t)Kf + 1);
}

TPSPP_EXPORT int tpspp_conv2d_bwd_weight(const float* const* src_ptrs, const int* src_dims, int nsrc, const float* dy,
                                         const float* y, int relu, int N, int Cout, int KH, int KW, int sh, int sw,
                                         int Ho, int Wo, float* dweight, float* dbias, float* ws, size_t ws_floats,
                                         tpspp_stream_t stream)
{
    const char* who = "tpspp_conv2d_bwd_weight";
    TPSPP_REQUIRE(src_ptrs && dy && (dweight || dbias), "%s: null pointer", who);
    TPSPP_REQUIRE(relu == 0 || relu == 1, "%s: activation code must be 0 (none) or 1 (ReLU)", who);
    TPSPP_REQUIRE(relu == 0 || y, "%s: null pointer (y is needed for the ReLU mask)", who);
    int Hi, Wi, Cin;
    const int rc = check_common(who, src_dims, nsrc, N, Cout, KH, KW, sh, sw, Ho, Wo, &Hi, &Wi, &Cin);
    if (rc != TPSPP_OK) return rc;
    for (int i = 0; i < nsrc; ++i) TPSPP_REQUIRE(src_ptrs[i], "%s: null pointer (source %d)", who, i);
    TPSPP_REQUIRE((Cout + 0LL) * Cin * KH * KW < (1LL << 31), "%s: weight too large", who);
    const size_t need = tpspp_conv2d_bwd_weight_workspace_floats(src_dims, nsrc, N, Cout, KH, KW, Ho, Wo);
    TPSPP_REQUIRE(ws_floats >= need && (need == 0 || ws),
                  "%s: ws too small (needs tpspp_conv2d_bwd_weight_workspace_floats(...) = %zu floats, got %zu)",
                  who, need, ws_floats);
    if (N == 0) return TPSPP_OK;
    BwdWeightParams P;
    P.nsrc = nsrc;
    for (int i = 0; i < 3; ++i) {
        const int j = i < nsrc ? i : nsrc - 1;
        const int* d = src_dims + 5 * j;
        P.src[i].p = src_ptrs[j];
        P.src[i].C = d[0]; P.src[i].H = d[1]; P.src[i].W = d[2]; P.src[i].uh = d[3]; P.src[i].uw = d[4];
    }
    P.dy = dy; P.y = relu ? y : nullptr; P.ws = ws;
    P.N = N; P.Cin = Cin; P.Cout = Cout; P.Hi = Hi; P.Wi = Wi; P.Ho = Ho; P.Wo = Wo; P.sh = sh; P.sw = sw;
    P.ph = (KH - 1) / 2; P.pw = (KW - 1) / 2;
    P.Kf = Cin * KH * KW;
    P.R = (long long)N * Ho * Wo;
    const SplitK k = split_k(P.R, Cout, P.Kf);
    P.chunks_per_slice = k.chunks_per_slice; P.S = k.S;
    P.want_db = dbias != nullptr;
    P.want_dw = dweight != nullptr;
    TPSPP_REQUIRE((Cout + BO - 1) / BO <= 65535, "%s: grid too large", who);
    hipStream_t st = tpspp::as_stream(stream);
    const dim3 grid(P.want_dw ? (unsigned)((P.Kf + BK - 1) / BK) : 1u, (unsigned)((Cout + BO - 1) / BO), (unsigned)k.S);
    if (KH == 1) hipLaunchKernelGGL(conv_bwd_weight_kernel<1>, grid, dim3(kThreads), 0, st, P);
    else         hipLaunchKernelGGL(conv_bwd_weight_kernel<3>, grid, dim3(kThreads), 0, st, P);
    int lr = tpspp::check_launch(who);
    if (lr != TPSPP_OK) return lr;
    const long long CK = (long long)Cout * P.Kf;
    const long long total = CK + Cout;
    hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const float*)ws, k.S, CK, Cout, dweight, dbias);
    return tpspp::check_launch("tpspp_conv2d_bwd_weight(reduce)");
}

// ------------------------------------------------------------------------------------------------------------------
// weight preparation for the forward of a training step: the weights change at every optimiser step, so the forward
// kernel's layouts are rebuilt on the device from PyTorch's (Cout, Cin, KH, KW) tensor
namespace {

__global__ void __launch_bounds__(256)
conv_prep_weight_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, int kc, int nch,
                        float* __restrict__ wt, float* __restrict__ tiled)
{
    // one thread per element of the (zero-padded) tiled layout [chunk][tap][ci-in-chunk][co]; wt (Cin*taps, Cout)
    const long long total = (long long)nch * taps * kc * Cout;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i % Cout);
    long long q = i / Cout;
    const int cl = (int)(q % kc); q /= kc;
    const int t = (int)(q % taps);
    const int ch = (int)(q / taps);
    const int ci = ch * kc + cl;
    const float v = ci < Cin ? w[((size_t)co * Cin + ci) * taps + t] : 0.0f;
    if (tiled) tiled[i] = v;
    if (wt && ci < Cin) wt[((size_t)ci * taps + t) * Cout + co] = v;
}

}  // namespace

TPSPP_EXPORT int tpspp_conv2d_prep_weight(const float* weight, int Cout, int Cin, int KH, int KW, float* weight_t,
                                          float* weight_tiled, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(weight && (weight_t || weight_tiled), "tpspp_conv2d_prep_weight: null pointer");
    TPSPP_REQUIRE((KH == 1 && KW == 1) || (KH == 3 && KW == 3), "tpspp_conv2d_prep_weight: kernel must be 1x1 or 3x3");
    TPSPP_REQUIRE(Cout > 0 && Cin > 0, "tpspp_conv2d_prep_weight: bad sizes");
    const int kc = tpspp_conv_chunk_channels(KH);
    const int nch = (Cin + kc - 1) / kc;
    const long long total = (long long)nch * KH * KW * kc * Cout;
    TPSPP_REQUIRE(total < (1LL << 31), "tpspp_conv2d_prep_weight: weight too large");
    hipLaunchKernelGGL(conv_prep_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       tpspp::as_stream(stream), weight, Cout, Cin, KH * KW, kc, nch, weight_t, weight_tiled);
    return tpspp::check_launch("tpspp_conv2d_prep_weight");
}
