// The recogniser head that consumes the rectified features: NRTR
// transformer encoder and greedy transformer decoder, fp32, one call per batch each.
//
// Replaces (reference, mmocr/models/): textrecog/encoders/nrtr_encoder.py:67-87,
// textrecog/decoders/nrtr_decoder.py:95-113,131-177, common/layers/transformer_layers.py:57-75,133-163,
// common/modules/transformer_module.py:24-33,75-99,119-125,155-163.
//
// Data layout: every activation is a CHANNEL-MAJOR matrix X[c][m] (row = feature, column = token,
// m = image*T + token for the encoder, m = image for one decoder step), i.e. exactly the (1, C, 1, M)
// "image" of a 1x1 convolution.  All projections therefore run on the library's fp32 MFMA
// convolution kernel (tpspp_conv.hip) with bias / GELU / residual fused in its epilogue and columns
// contiguous in every load and store; the encoder's NCHW input needs one re-layout on entry.  Where a
// consumer wants TOKEN-major rows (the decoder's q/k/v of one step, the cross-attention values) the
// same kernel is called with the operands swapped (the activation as its "weights", the prepared
// weight as its "image"): D[m][cout] instead of D[cout][m], no transpose kernel.
//
// The decoder is incremental: the reference re-runs the whole padded target (41 positions) through all
// layers at each of its 40 steps and keeps one row; with a causal mask that row depends only on earlier
// positions, so one position per step against cached self-attention keys/values gives the same numbers
// (up to summation order) with 1/41 of the arithmetic.  The encoder keys/values of the cross attention
// are projected once per layer.  The whole loop is enqueued without host synchronisation: the arg-max
// of step s is written to a device token buffer that step s+1's embedding kernel reads.
//
// Bounds: projections: MFMA (fp32 matrix rate); LayerNorm / attention kernels: HBM / L2 (one pass over
// their operands), LDS-broadcast reads in the encoder attention.
#include <cmath>

#include "tpspp_common.h"

#include <mutex>
#include "tpspp_tokgemm.h"
#include "tpspp_dev.h"

#include <cstdlib>

using namespace tpspp_dev;

namespace {

#include "tpspp_head_kernels.h"
#include "tpspp_head_step.h"

// ---- host side ---------------------------------------------------------------------------------------------------
long long* g_head_trace = nullptr;     // tpspp_head_set_trace

// the projections outside the decoder's steps, as 1x1 convolutions / token GEMMs; the first failure sticks in `rc`
struct Gemm {
    hipStream_t st;
    int rc = 0;
    int b16 = 0, split3 = 0;           // what proj() runs on: 0, 0 the fp32 matrix cores; 1, 0 bf16; 1, 1 the three-term split
    // the same product on the bf16 matrix cores: W16 = the weight arranged for tpspp_conv2d_bf16_fwd (1x1),
    // X / res fp32 (rounded to bf16 as they are staged), out fp32 or bf16
    // split3: the "bf16x3" three-term split on the fp32 operands (W16 then holds hi and lo slabs)
    void cm16(const void* W16, const float* bias, const float* X, int K, int Co, int M, void* out, int out_f32, int act,
              const float* res, int split3 = 0)
    {
        if (rc) return;
        // the token GEMM (tpspp_tokgemm.hip) where the shape qualifies, else the product as a 1x1 convolution
        tpspp::TokGemmArgs ta;
        ta.X = X; ta.W = W16; ta.bias = bias; ta.res = res; ta.out = out; ta.out_f32 = out_f32;
        ta.K = K; ta.Co = Co; ta.M = M; ta.act = act; ta.x3 = split3; ta.kgc = tpspp_conv_bf16_chunk_channels(1) / 8;
        if (tpspp::tok_gemm_applicable(ta)) {
            tpspp::launch_tok_gemm(ta, st);
            rc = tpspp::check_launch("token GEMM");
            return;
        }
        const void* src[1] = {X};
        const int dims[6] = {K, 1, M, 1, 1, 1};
        rc = tpspp_conv2d_bf16_fwd(src, dims, 1, W16, bias, res, 1, nullptr, nullptr, res ? 1 : 0, act, 1, Co, 1, 1, 1, 1,
                                   out, out_f32, 1, M, split3, st);
    }
    // out (Co, M) = act(W^T X + bias) [+ res]      W (K, Co) k-major, X (K, M) channel-major
    void cm(const float* W, const float* bias, const float* X, int K, int Co, int M, float* out, int act,
            const float* res)
    {
        if (rc) return;
        const float* src[1] = {X};
        const int dims[5] = {K, 1, M, 1, 1};
        rc = tpspp_conv2d_fwd(src, dims, 1, W, (K % 32 == 0) ? W : nullptr, bias, res, nullptr, nullptr,
                              res ? 1 : 0, act, 1, Co, 1, 1, 1, 1, out, 1, M, st);
    }
    // cm() or cm16() with an fp32 result, by the precision this Gemm was made with (W in that precision's form)
    void proj(const float* W, const float* bias, const float* X, int K, int Co, int M, float* out, int act,
              const float* res)
    {
        if (b16) cm16(W, bias, X, K, Co, M, out, 1, act, res, split3);
        else cm(W, bias, X, K, Co, M, out, act, res);
    }
    // out (M, Co) token-major = X^T W           (operands swapped: X plays the weights, W the image)
    void tm(const float* W, const float* X, int K, int Co, int M, float* out)
    {
        if (rc) return;
        const float* src[1] = {W};
        const int dims[5] = {K, 1, Co, 1, 1};
        rc = tpspp_conv2d_fwd(src, dims, 1, X, (K % 32 == 0) ? X : nullptr, nullptr, nullptr, nullptr, nullptr,
                              0, 0, 1, M, 1, 1, 1, 1, out, 1, Co, st);
    }
};

// ---- workspace layouts --------------------------------------------------------------------------------------------
// EncWorkspace / DecWorkspace::layout() is the one statement of what a workspace holds: it walks the buffers in order,
// each aligned to 256 bytes.  With a null base it only counts (`bytes` is what the *_workspace queries report and what
// the entry points ask of the caller), with the caller's pointer the members are the buffers.
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Walk {
    char* base;
    size_t off = 0;
    char* raw(size_t bytes)
    {
        char* r = base ? base + off : nullptr;
        off += align256(bytes);
        return r;
    }
    float* f(size_t n) { return reinterpret_cast<float*>(raw(n * sizeof(float))); }
};

struct EncWorkspace {
    float *x, *y, *a, *qkv, *hid;
    size_t bytes;
    void layout(void* base, int N, int C, int T, int Di)
    {
        const size_t M = (size_t)N * T;
        Walk w{static_cast<char*>(base)};
        x = w.f((size_t)C * M);
        y = w.f((size_t)C * M);
        a = w.f((size_t)C * M);
        qkv = w.f((size_t)3 * C * M);
        hid = w.f((size_t)Di * M);
        bytes = w.off;
    }
};

// the persistent step kernel's counter block: one counter per cluster of 32 images, 128 B apart, then the error flag
constexpr size_t kDecErrWords = 64;
inline size_t dec_counter_words(int N) { return (size_t)(N + 31) / 32 * 32 + kDecErrWords; }

struct DecWorkspace {
    char* layers;                      // per layer Kx | Vx | Kc | Vc: Kx(l) .. Vc(l)
    size_t kx_bytes, kc_bytes;
    float *x, *y, *a, *qkv, *hid, *logits;
    int* tokens;
    float* ktmp;                       // keys before their transposition (token-major step pipeline)
    int *counters, *err;               // dec_counter_words(N) words: the cluster counters, the error flag behind them
    size_t bytes;
    void layout(void* base, int N, int C, int T, int Di, int n_layers, int L, int Cc)
    {
        const size_t MT = (size_t)N * T;
        Walk w{static_cast<char*>(base)};
        kx_bytes = align256((size_t)C * MT * 4);                  // encoder keys / values (token-major; the bf16 head uses
                                                                  // the upper half of a slot as staging)
        kc_bytes = align256((size_t)N * C * (size_t)L * 4);       // self-attention caches
        layers = w.raw((size_t)n_layers * (2 * kx_bytes + 2 * kc_bytes));
        x = w.f((size_t)C * N);
        y = w.f((size_t)C * N);
        a = w.f((size_t)C * N);
        qkv = w.f((size_t)3 * C * N);
        hid = w.f((size_t)Di * N);
        logits = w.f((size_t)Cc * N);
        tokens = reinterpret_cast<int*>(w.f((size_t)N * (L + 1)));
        ktmp = w.f((size_t)C * MT);
        counters = reinterpret_cast<int*>(w.f(dec_counter_words(N)));
        err = counters ? counters + (dec_counter_words(N) - kDecErrWords) : nullptr;
        bytes = w.off;
    }
    char* layer(int l) const { return layers + (size_t)l * (2 * kx_bytes + 2 * kc_bytes); }
    float* Kx(int l) const { return reinterpret_cast<float*>(layer(l)); }
    float* Vx(int l) const { return reinterpret_cast<float*>(layer(l) + kx_bytes); }
    float* Kc(int l) const { return reinterpret_cast<float*>(layer(l) + 2 * kx_bytes); }
    float* Vc(int l) const { return reinterpret_cast<float*>(layer(l) + 2 * kx_bytes + kc_bytes); }
};

// layer pointer tables: see include/tpspp.h
enum { E_LN1G, E_LN1B, E_WQKV, E_BQKV, E_WFC, E_BFC, E_LN2G, E_LN2B, E_W1, E_B1, E_W2, E_B2, E_COUNT };
// decoder: the three LayerNorms are folded into the projections that follow them (tpspp_linear_ln_fwd)
enum { D_QKV_W, D_QKV_CS, D_QKV_B, D_WFC, D_BFC, D_Q_W, D_Q_CS, D_Q_B, D_WK, D_BK, D_WV, D_WFC2, D_BFC2, D_W1_W, D_W1_CS,
       D_W1_B, D_W2, D_B2,
       // the six per-step projections arranged for the step GEMM: split hi / lo bf16 (TPSPP_HEAD_BF16 / _BF16X3) or fp32
       D_QKV_X, D_WFC_X, D_Q_X, D_WFC2_X, D_W1_X, D_W2_X, D_COUNT };

// ---- the decoder's route: which pipeline and which kernels a decode takes, as a value -------------------------------------
// dec_route() holds every condition that depends on sizes, flags and the table alone; tpspp_nrtr_decoder_fwd consumes only
// its result, and tpspp_nrtr_decoder_route reports it (a host-side query, so that a test can pin the dispatch).  What the
// DEVICE adds for a persistent-eligible route -- co-residency, stream capture, the environment switches -- is a second
// step in the entry point (persist_groups_now).
enum { kDecPlain = 0, kDecArranged = 1, kDecPersistent = 2 };

struct DecRoute {
    int pipeline;     // kDecPlain: channel-major steps on tpspp_linear_ln_fwd + the convolution kernel;
                      // kDecArranged: token-major steps on the step GEMM, ~50 launches per step;
                      // kDecPersistent: eligible for ONE persistent launch per decode, else as kDecArranged
    bool kv16;        // encoder keys / values and the self-attention caches as bf16 (TPSPP_HEAD_BF16), else fp32
    bool gemm_f32;    // step GEMM and key projection with exact fp32 products, else the three-term bf16 split
    bool cross2;      // kDecArranged: cross-attention with two heads per wavefront, else one
    int persist;      // kDecPersistent: index into kPersistKernels and PersistDevice::groups, else -1
};

// the step GEMM has an instantiation for this (K, Co): dec_route() admits the step pipelines on it, StepGemm holds to it
bool dec_gemm_has_kernel(int K, int Co) { return (K == 256 || K == 512) && (Co & 3) == 0; }

// every layer's six arranged projections and the arranged classifier (behind the layers) are in the table
bool dec_table_arranged(const float* const* layer_ptrs, int n_layers)
{
    if (!layer_ptrs[(size_t)n_layers * D_COUNT]) return false;
    for (int l = 0; l < n_layers; ++l) {
        const float* const* w = layer_ptrs + (size_t)l * D_COUNT;
        if (!(w[D_QKV_X] && w[D_WFC_X] && w[D_Q_X] && w[D_WFC2_X] && w[D_W1_X] && w[D_W2_X])) return false;
    }
    return true;
}

DecRoute dec_route(int C, int T, int d_inner, int n_layers, int num_out, int flags, bool arranged)
{
    const int H = C / kDK;
    DecRoute R;
    R.kv16 = (flags & TPSPP_HEAD_BF16) != 0;                                      // (wins over _BF16X3)
    R.gemm_f32 = !R.kv16 && (flags & TPSPP_HEAD_BF16X3) == 0;
    // Arranged per-step weights in the table (whatever the flags: they are fp32 fragments for the exact-fp32 head, hi / lo
    // bf16 for the other two) and a kernel for each of the seven products: every activation of a step is TOKEN-major and
    // the six projections + the classifier run on the step GEMM.
    const bool steps = arranged && dec_gemm_has_kernel(C, 3 * C) && dec_gemm_has_kernel(C, C) &&
                       dec_gemm_has_kernel(C, d_inner) && dec_gemm_has_kernel(d_inner, C) && dec_gemm_has_kernel(C, num_out);
    // the step as ONE persistent launch (tpspp_head_persist.h): every head configuration, d_model 512, 8 heads
    const bool persistent = steps && C == 512 && H == 8 && num_out <= 128 && n_layers <= kPMaxLayers;
    R.pipeline = persistent ? kDecPersistent : steps ? kDecArranged : kDecPlain;
    // two heads per wavefront (round 5): both heads' keys, then both heads' values in flight together
    R.cross2 = steps && T <= kWave && (H & 1) == 0;
    // more than 64 encoder tokens: the kernel's other instantiation (TBIG)
    R.persist = persistent ? (T > kWave ? 6 : 0) + (R.kv16 ? 2 : R.gemm_f32 ? 4 : 0) + (d_inner == 256 ? 0 : 1) : -1;
    return R;
}

// dec_step_persist_kernel<KV, d_inner / 128, exact fp32, TBIG> by DecRoute::persist
using PersistKernel = void (*)(const PStep);
const PersistKernel kPersistKernels[12] = {
    dec_step_persist_kernel<float, 2, false>,                dec_step_persist_kernel<float, 4, false>,
    dec_step_persist_kernel<unsigned short, 2, false>,       dec_step_persist_kernel<unsigned short, 4, false>,
    dec_step_persist_kernel<float, 2, true>,                 dec_step_persist_kernel<float, 4, true>,
    dec_step_persist_kernel<float, 2, false, true>,          dec_step_persist_kernel<float, 4, false, true>,
    dec_step_persist_kernel<unsigned short, 2, false, true>, dec_step_persist_kernel<unsigned short, 4, false, true>,
    dec_step_persist_kernel<float, 2, true, true>,           dec_step_persist_kernel<float, 4, true, true>,
};

// ---- the step GEMM's launches --------------------------------------------------------------------------------------
template <typename P>
P dec_gemm_params(const float* X, const void* Wp, const float* bias, const float* colsum, float eps, const float* res,
                  int act, int M, int K, int Co, float* out, int remap)
{
    P p;
    p.X = X; p.Wp = reinterpret_cast<decltype(p.Wp)>(Wp); p.bias = bias; p.colsum = colsum; p.res = res; p.out = out;
    p.M = M; p.K = K; p.Co = Co; p.eps = eps; p.act = act; p.remap = remap;
    return p;
}

// the token-major projections of one decode: out (M, Co) = act(LN?(X) Wp + bias) [+ res]; the first failure sticks in `rc`
struct StepGemm {
    hipStream_t st;
    int M;
    bool f32;          // exact fp32 products (dec_gemm_f32_kernel), else the three-term split (dec_gemm_x3_kernel)
    int rc = 0;
    void operator()(const float* X, const void* Wp, const float* bias, const float* colsum, float eps, const float* res,
                    int act, int K, int Co, float* out)
    {
        if (rc) return;
        if (!dec_gemm_has_kernel(K, Co)) {
            rc = tpspp::fail(TPSPP_EINVAL, "tpspp_nrtr_decoder_fwd: no step GEMM for K = %d, Co = %d", K, Co);
            return;
        }
        const dim3 grid((unsigned)((M + 31) / 32), (unsigned)((Co + 31) / 32));
        const bool ln = colsum != nullptr;
        if (f32) {
            const DGemmF P = dec_gemm_params<DGemmF>(X, Wp, bias, colsum, eps, res, act, M, K, Co, out, 0);   // (remap measured: nothing for the exact-fp32 form)
            if (K == 512) {
                if (ln) hipLaunchKernelGGL((dec_gemm_f32_kernel<8, true>), grid, dim3(512), 0, st, P);
                else    hipLaunchKernelGGL((dec_gemm_f32_kernel<8, false>), grid, dim3(512), 0, st, P);
            } else {
                if (ln) hipLaunchKernelGGL((dec_gemm_f32_kernel<4, true>), grid, dim3(512), 0, st, P);
                else    hipLaunchKernelGGL((dec_gemm_f32_kernel<4, false>), grid, dim3(512), 0, st, P);
            }
            return;
        }
        const DGemm P = dec_gemm_params<DGemm>(X, Wp, bias, colsum, eps, res, act, M, K, Co, out, 1);
        // the q|k|v projection (1536 outputs, folded LayerNorm) of the three-term form: three tiles per workgroup, one round of
        // 256 workgroups instead of 768 in two (bf16x3 decoder 20.85 -> 20.45 ms, bf16 15.68 -> 15.33 against one tile per
        // workgroup, bit-identical scores).  Not the exact-fp32 form: its 96 fp32 matrix instructions per wavefront are the
        // launch's time either way (23.40 -> 23.72 ms with three tiles).
        if (K == 512 && ln && Co >= 1024) {
            const dim3 grid3((unsigned)((M + 31) / 32), (unsigned)(((Co + 31) / 32 + 2) / 3));
            hipLaunchKernelGGL((dec_gemm_x3_kernel<8, true, 3>), grid3, dim3(256), 0, st, P);
        } else if (K == 512) {
            if (ln) hipLaunchKernelGGL((dec_gemm_x3_kernel<8, true>), grid, dim3(256), 0, st, P);
            else    hipLaunchKernelGGL((dec_gemm_x3_kernel<8, false>), grid, dim3(256), 0, st, P);
        } else {
            if (ln) hipLaunchKernelGGL((dec_gemm_x3_kernel<4, true>), grid, dim3(256), 0, st, P);
            else    hipLaunchKernelGGL((dec_gemm_x3_kernel<4, false>), grid, dim3(256), 0, st, P);
        }
    }
};

// ---- one decode: what its parts share ------------------------------------------------------------------------------------
struct DecCtx {
    hipStream_t st;
    tpspp_stream_t stream;             // the same stream, as the library's own entry points take it
    int N, C, T, H, d_inner, n_layers, num_out, L, Lt;
    const float* enc_cm;
    const float* const* layer_ptrs;
    const void* cls_x;                 // the classifier, arranged (behind the layers), or NULL
    const float *emb, *pos_table, *w_cls, *cls_colsum, *b_cls;
    int padding_idx, greedy;
    const int* valid_len;
    float* out;
    DecWorkspace W;
    DecRoute R;
    const float* const* layer(int l) const { return layer_ptrs + (size_t)l * D_COUNT; }
    unsigned pair_blocks() const { return (unsigned)((N * H + 3) / 4); }      // a wavefront per (image, head), four per workgroup
};

// calls f<KV>(c) with the route's key / value element type
#define TPSPP_HEAD_KV(c, f) ((c).R.kv16 ? f<unsigned short>(c) : f<float>(c))

template <typename KV> KV* kv_ptr(float* p) { return reinterpret_cast<KV*>(p); }

// x (token-major: N, C; else C, N) = embedding of every image's token of step s + the position's row
void launch_embed(const DecCtx& c, int s, float* x, int token_major)
{
    hipLaunchKernelGGL(dec_embed_kernel, dim3((unsigned)((c.C * c.N + 255) / 256)), dim3(256), 0, c.st, c.emb, c.pos_table,
                       c.W.tokens, c.Lt, s, c.C, c.N, x, token_major);
}

// a = self-attention of step s against layer l's caches (and appends to them); out_cm: a channel-major
template <typename KV>
void launch_self_attn(const DecCtx& c, int l, int s, int out_cm)
{
    hipLaunchKernelGGL(attn_dec_self_wide_kernel<KV>, dim3(c.pair_blocks()), dim3(256), 0, c.st, c.W.qkv, c.C, c.N, c.H, s, c.L,
                       kv_ptr<KV>(c.W.Kc(l)), kv_ptr<KV>(c.W.Vc(l)), c.W.tokens, c.Lt, c.padding_idx, c.W.a, out_cm);
}

// a = cross-attention of the q rows in qkv against layer l's encoder keys / values, one head per wavefront
template <typename KV>
void launch_cross_attn(const DecCtx& c, int l, int out_cm)
{
    hipLaunchKernelGGL(attn_dec_cross_wide_kernel<KV>, dim3(c.pair_blocks()), dim3(256), 0, c.st, c.W.qkv,
                       kv_ptr<const KV>(c.W.Kx(l)), kv_ptr<const KV>(c.W.Vx(l)), c.C, c.N, c.H, c.T, c.valid_len, c.W.a, out_cm);
}

// the same with two heads per wavefront (DecRoute::cross2; token-major)
template <typename KV>
void launch_cross_attn2(const DecCtx& c, int l)
{
    const unsigned blocks2 = (unsigned)((c.N * (c.H / 2) + 3) / 4);
    hipLaunchKernelGGL(attn_dec_cross_wide2_kernel<KV>, dim3(blocks2), dim3(256), 0, c.st, c.W.qkv, c.C,
                       kv_ptr<const KV>(c.W.Kx(l)), kv_ptr<const KV>(c.W.Vx(l)), c.C, c.N, c.H, c.T, c.valid_len, c.W.a);
}

// encoder keys and values (both token-major) of every layer, once per decode
template <typename KV>
int project_encoder_kv(const DecCtx& c)
{
    const int C = c.C, MT = c.N * c.T;
    const bool x3 = !c.R.kv16 && !c.R.gemm_f32;
    Gemm g{c.st, 0, x3, x3};                               // (proj: the fp32 keys, exact or by the three-term split)
    for (int l = 0; l < c.n_layers; ++l) {
        const float* const* w = c.layer(l);
        if constexpr (sizeof(KV) == 2) {
            // bf16 matrix cores, bf16 keys / values: both channel-major straight from the epilogue into the upper half of
            // their own (fp32-sized) slot, then transposed to token-major rows
            KV* vt = kv_ptr<KV>(c.W.Vx(l)) + (size_t)C * MT;
            KV* kt = kv_ptr<KV>(c.W.Kx(l)) + (size_t)C * MT;
            g.cm16(w[D_WK], w[D_BK], c.enc_cm, C, C, MT, kt, 0, 0, nullptr);
            g.cm16(w[D_WV], nullptr, c.enc_cm, C, C, MT, vt, 0, 0, nullptr);
            if (g.rc) return g.rc;
            const dim3 grid((unsigned)((MT + 63) / 64), (unsigned)((C + 63) / 64));
            hipLaunchKernelGGL(transpose2d_b16_kernel, grid, dim3(256), 0, c.st, reinterpret_cast<unsigned short*>(vt), C, MT,
                               reinterpret_cast<unsigned short*>(c.W.Vx(l)));
            hipLaunchKernelGGL(transpose2d_b16_kernel, grid, dim3(256), 0, c.st, reinterpret_cast<unsigned short*>(kt), C, MT,
                               reinterpret_cast<unsigned short*>(c.W.Kx(l)));
        } else {
            g.proj(w[D_WK], w[D_BK], c.enc_cm, C, C, MT, c.W.ktmp, 0, nullptr);
            if (g.rc) return g.rc;
            // (C, N*T) -> (N*T, C): the wide-load cross-attention's layout
            if (int rc = tpspp_transpose2d(c.W.ktmp, C, MT, c.W.Kx(l), c.stream)) return rc;
            g.tm(w[D_WV], c.enc_cm, C, C, MT, c.W.Vx(l));  // (a value bias would be per channel = per column here: not supported)
        }
    }
    return g.rc;
}

// ---- the persistent decode's two requirements (include/tpspp.h, tpspp_nrtr_decoder_fwd) -----------------------------------
// (1) Co-residency.  The 16 workgroups of a cluster spin on each other's counter, and blocks are dispatched in order: a launch
//     makes progress iff a whole GROUP of 8 clusters (128 consecutive blocks) can be resident.  persist_groups() = how many such
//     groups the device holds at once (CU count x the kernel's occupancy at 512 threads + sizeof(PShared) of LDS, / 128), capped
//     at 2 (512 images per launch); 0 -- a smaller part, a CU-masked or CPX partition, a failed attribute call -- sends the
//     decode down the launch-per-phase pipeline.
// (2) One persistent decode in flight per device.  Two of them on two streams are harmless by themselves (in-order dispatch:
//     one of them always owns a whole group), three can starve each other until the timeout; instead of reasoning about the
//     dispatcher, every persistent decode waits (hipStreamWaitEvent, no host synchronisation) for the event recorded behind
//     the previous one on this device, whatever its stream, and records its own.  Decodes of one process therefore never
//     overlap each other on a device; kernels of other streams may overlap them freely (they finish on their own, the barrier
//     timeout is wall-clock time).  Other PROCESSES on the same device are not seen by this guard: one process per GPU.
struct PersistDevice {
    hipEvent_t done = nullptr;
    bool recorded = false;
    int groups[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};      // per kernel instantiation; -1 = not queried yet
};
std::mutex g_persist_mu;
PersistDevice g_persist_dev[tpspp::kMaxDevices];

int persist_groups(PersistDevice& D, int which, int dev)
{
    if (D.groups[which] < 0) {
        const PersistKernel kern = kPersistKernels[which];
        int groups = 0, cus = 0, per_cu = 0;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PShared)) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 512, sizeof(PShared)) == hipSuccess) {
            groups = (int)(((long)cus * per_cu) / 128);
            if (groups > 2) groups = 2;
        }
        (void)hipGetLastError();
        D.groups[which] = groups;
    }
    return D.groups[which];
}

// The environment switches of the persistent path, all read here, once per persistent-eligible decode (per call: tests set
// and unset them between calls).
struct PersistEnv {
    bool no_persist;       // TPSPP_HEAD_NO_PERSIST=1: the reduced-precision step pipeline as ~50 launches per step (rounds 3-4)
                           // instead of ONE persistent launch per decode; bit-identical scores -- for A/B runs and the bit-identity test
    int groups_cap;        // TPSPP_HEAD_PERSIST_GROUPS (lab / test switch): pretend the device holds fewer groups; -1 = unset
    int write_through;     // TPSPP_HEAD_WRITE_THROUGH (lab / test switch): PStep::no_plain
    int timeout_k;         // TPSPP_HEAD_TIMEOUT_MS: barrier timeout, wall-clock milliseconds (default 4000) -> units of 1024
                           // ticks of the 100 MHz clock
    int test_stall_step;   // TPSPP_HEAD_TEST_STALL (test hook): PStep::test_stall_step; -1 = off
};

PersistEnv read_persist_env()
{
    PersistEnv E;
    E.no_persist = getenv("TPSPP_HEAD_NO_PERSIST") != nullptr;
    const char* v = getenv("TPSPP_HEAD_PERSIST_GROUPS");
    E.groups_cap = v ? atoi(v) : -1;
    E.write_through = getenv("TPSPP_HEAD_WRITE_THROUGH") ? 1 : 0;
    v = getenv("TPSPP_HEAD_TIMEOUT_MS");
    const long ms = v ? atol(v) : 4000;
    E.timeout_k = (int)((ms < 1 ? 1 : ms > 60000 ? 60000 : ms) * 100000 / 1024);
    v = getenv("TPSPP_HEAD_TEST_STALL");
    E.test_stall_step = v ? atoi(v) : -1;
    return E;
}

// The device's word on a persistent-eligible route: the groups of clusters a launch may hold (requirement (1)), 0 = take
// the launch pipeline -- also under stream capture (the in-flight guard's events would become graph nodes).
int persist_groups_now(const DecCtx& c, const PersistEnv& E, int& dev)
{
    if (E.no_persist) return 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= tpspp::kMaxDevices ||
        hipStreamIsCapturing(c.st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_persist_mu);
    int groups = persist_groups(g_persist_dev[dev], c.R.persist, dev);
    if (E.groups_cap >= 0 && E.groups_cap < groups) groups = E.groups_cap;
    return groups;
}

// everything of the persistent kernel's argument that does not change between the launches of a decode
PStep persist_step(const DecCtx& c, const PersistEnv& E)
{
    PStep PS;
    for (int l = 0; l < c.n_layers; ++l) {
        const float* const* w = c.layer(l);
        PLayer& q = PS.L[l];
        q.qkv_x = w[D_QKV_X]; q.wfc_x = w[D_WFC_X]; q.q_x = w[D_Q_X]; q.wfc2_x = w[D_WFC2_X]; q.w1_x = w[D_W1_X]; q.w2_x = w[D_W2_X];
        q.qkv_cs = w[D_QKV_CS]; q.qkv_b = w[D_QKV_B]; q.bfc = w[D_BFC]; q.q_cs = w[D_Q_CS]; q.q_b = w[D_Q_B];
        q.bfc2 = w[D_BFC2]; q.w1_cs = w[D_W1_CS]; q.w1_b = w[D_W1_B]; q.b2 = w[D_B2];
        q.Kx = c.W.Kx(l); q.Vx = c.W.Vx(l); q.Kc = c.W.Kc(l); q.Vc = c.W.Vc(l);
    }
    PS.n_layers = c.n_layers;
    PS.x = c.W.x; PS.y = c.W.y; PS.a = c.W.a; PS.qkv = c.W.qkv; PS.hid = c.W.hid; PS.logits = c.W.logits;
    PS.cls_x = c.cls_x; PS.cls_cs = c.cls_colsum; PS.cls_b = c.b_cls; PS.num_out = c.num_out;
    PS.emb = c.emb; PS.pos = c.pos_table; PS.tokens = c.W.tokens; PS.Lt = c.Lt; PS.out = c.out; PS.greedy = c.greedy;
    PS.pad_idx = c.padding_idx;
    PS.valid_len = c.valid_len; PS.N = c.N; PS.C = c.C; PS.T = c.T; PS.H = c.H; PS.d_inner = c.d_inner;
    PS.step = 0; PS.nsteps = c.L; PS.Lsteps = c.L; PS.Lmax = c.L; PS.bar_base = 0;
    PS.err = c.W.err;
    PS.pairs = 2;
    PS.trace = g_head_trace;
    PS.no_plain = E.write_through;
    PS.timeout_k = E.timeout_k;
    PS.test_stall_step = E.test_stall_step;
    // odd clusters start 15 us late (against all together: bf16x3 20.0 -> 19.4 ms, bf16 15.4 -> 15.0)
    PS.stagger = (c.N > 32 ? 15 : 0) * 100;
    return PS;
}

// the steps as persistent launches of `groups` x 256 images (tpspp_head_persist.h), with the copy-outs behind them
int decode_persistent(const DecCtx& c, const PersistEnv& E, int dev, int groups, int* tokens_out, int* status_out)
{
    PStep PS = persist_step(c, E);
    const size_t counter_bytes = dec_counter_words(c.N) * sizeof(int);
    // requirement (2): behind the previous persistent decode of this device, whatever stream it ran on
    std::lock_guard<std::mutex> lk(g_persist_mu);
    PersistDevice& PD = g_persist_dev[dev];
    if (!PD.done && hipEventCreateWithFlags(&PD.done, hipEventDisableTiming) != hipSuccess)
        return tpspp::check_launch("tpspp_nrtr_decoder_fwd(event)");
    if (PD.recorded && hipStreamWaitEvent(c.st, PD.done, 0) != hipSuccess)
        return tpspp::check_launch("tpspp_nrtr_decoder_fwd(wait for the previous persistent decode)");
    if (hipMemsetAsync(c.W.counters, 0, counter_bytes, c.st) != hipSuccess)
        return tpspp::check_launch("tpspp_nrtr_decoder_fwd(memset)");
    launch_embed(c, 0, c.W.x, 1);
    // ONE launch per decode: the kernel loops over the steps, clusters run their 40 steps independently of each other.
    // (With the clusters spread over the XCDs -- the first version of this kernel -- one launch per step was faster:
    // 23.04 against 23.25 ms; with a cluster per XCD and ordinary stores the step loop inside wins: fp32 22.12 -> 21.58 ms,
    // bf16x3 19.67 -> 19.07, bf16 14.29 -> 13.83 at batch 512.)
    const int img_per_launch = 256 * groups;               // every cluster of a launch resident: `groups` x 8 clusters x 32 images
    for (int n0 = 0; n0 < c.N; n0 += img_per_launch) {
        const int nimg = c.N - n0 < img_per_launch ? c.N - n0 : img_per_launch;
        PS.n0 = n0; PS.counters = c.W.counters + (n0 >> 5) * 32;
        PS.nclusters = (nimg + 31) / 32;
        // cluster c = 8 j + x is the 16 blocks 8 (16 j + ct) + x: one XCD per cluster (see the kernel)
        hipLaunchKernelGGL(kPersistKernels[c.R.persist], dim3((unsigned)((PS.nclusters + 7) / 8 * 128)), dim3(512), sizeof(PShared),
                           c.st, PS);
    }
    const hipError_t rec = hipEventRecord(PD.done, c.st);
    PD.recorded = PD.recorded || rec == hipSuccess;
    if (tokens_out)
        (void)hipMemcpyAsync(tokens_out, c.W.tokens, (size_t)c.N * c.Lt * sizeof(int), hipMemcpyDeviceToDevice, c.st);
    if (status_out)
        (void)hipMemcpyAsync(status_out, PS.err, sizeof(int), hipMemcpyDeviceToDevice, c.st);
    return tpspp::check_launch("tpspp_nrtr_decoder_fwd(persistent step)");
}

// Reduced-precision or exact head with arranged per-step weights in the table: every activation of a step is TOKEN-major
// and the six projections + the classifier run on the step GEMM.  8 launches per layer-step, each about half as long as
// the plain pipeline's.
template <typename KV>
int decode_steps_arranged(const DecCtx& c)
{
    const int N = c.N, C = c.C, Di = c.d_inner;
    float *x = c.W.x, *y = c.W.y;
    float* const a = c.W.a;
    float* const qkv = c.W.qkv;
    StepGemm gemm{c.st, N, c.R.gemm_f32};
    launch_embed(c, 0, x, 1);
    for (int s = 0; s < c.L; ++s) {
        for (int l = 0; l < c.n_layers; ++l) {
            const float* const* w = c.layer(l);
            gemm(x, w[D_QKV_X], w[D_QKV_B], w[D_QKV_CS], 1e-5f, nullptr, 0, C, 3 * C, qkv);
            launch_self_attn<KV>(c, l, s, 0);
            gemm(a, w[D_WFC_X], w[D_BFC], nullptr, 0.0f, x, 0, C, C, y);                     // y = x + fc(a)
            // (q projection and cross-attention as two launches: fused into one they measured slower, bf16x3 decoder 24.9
            // against 21.8 ms, bf16 18.05 against 16.65 ms at batch 512 -- DESIGN.md)
            gemm(y, w[D_Q_X], w[D_Q_B], w[D_Q_CS], 1e-5f, nullptr, 0, C, C, qkv);
            if (c.R.cross2) launch_cross_attn2<KV>(c, l);
            else launch_cross_attn<KV>(c, l, 0);
            gemm(a, w[D_WFC2_X], w[D_BFC2], nullptr, 0.0f, y, 0, C, C, x);                   // x = y + fc(a)
            gemm(x, w[D_W1_X], w[D_W1_B], w[D_W1_CS], 1e-5f, nullptr, 2, C, Di, c.W.hid);
            gemm(c.W.hid, w[D_W2_X], w[D_B2], nullptr, 0.0f, x, 0, Di, C, y);                // y = x + w2(...)
            float* t = x; x = y; y = t;
        }
        gemm(x, c.cls_x, c.b_cls, c.cls_colsum, 1e-6f, nullptr, 0, C, c.num_out, c.W.logits);
        if (gemm.rc) return gemm.rc;
        // (x holds this step's final activations, read by the classifier launch above; the next step's embedding goes to y,
        //  which becomes x)
        const bool more = s + 1 < c.L;
        hipLaunchKernelGGL(dec_classify_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c.st, c.W.logits, c.num_out,
                           N, s, c.L, c.greedy, c.out, c.W.tokens, c.Lt, 1, c.emb, c.pos_table, more ? y : nullptr, C);
        if (more) { float* t = x; x = y; y = t; }
    }
    return TPSPP_OK;
}

// No arranged weights (or a shape the step GEMM has no kernel for): channel-major activations, the LayerNorm-folded
// projections on tpspp_linear_ln_fwd, the others on the convolution kernel.
template <typename KV>
int decode_steps_plain(const DecCtx& c)
{
    const int N = c.N, C = c.C, Di = c.d_inner;
    float *x = c.W.x, *y = c.W.y;
    float* const a = c.W.a;
    float* const qkv = c.W.qkv;
    Gemm g{c.st};
    int rc = 0;
    for (int s = 0; s < c.L; ++s) {
        launch_embed(c, s, x, 0);
        for (int l = 0; l < c.n_layers; ++l) {
            const float* const* w = c.layer(l);
            // x = x + fc(self_attn(LN1(x)))                          transformer_layers.py:150-154
            rc = tpspp_linear_ln_fwd(x, C, N, 1e-5f, w[D_QKV_W], w[D_QKV_CS], 3 * C, w[D_QKV_B], 0, nullptr, 1, qkv, c.stream);
            if (rc) return rc;
            launch_self_attn<KV>(c, l, s, 1);
            g.cm(w[D_WFC], w[D_BFC], a, C, C, N, y, 0, x);            // y = x + fc(a)
            // x = y + fc(enc_attn(LN2(y), enc, enc))                   transformer_layers.py:156-159
            rc = tpspp_linear_ln_fwd(y, C, N, 1e-5f, w[D_Q_W], w[D_Q_CS], C, w[D_Q_B], 0, nullptr, 1, qkv, c.stream);
            if (rc) return rc;
            launch_cross_attn<KV>(c, l, 1);
            g.cm(w[D_WFC2], w[D_BFC2], a, C, C, N, x, 0, y);          // x = y + fc(a)
            // x = x + mlp(LN3(x))                                       transformer_layers.py:161-163
            rc = tpspp_linear_ln_fwd(x, C, N, 1e-5f, w[D_W1_W], w[D_W1_CS], Di, w[D_W1_B], 2, nullptr, 0, c.W.hid, c.stream);
            if (rc) return rc;
            g.cm(w[D_W2], w[D_B2], c.W.hid, Di, C, N, y, 0, x);       // y = x + w2(...)
            float* t = x; x = y; y = t;
            if (g.rc) return g.rc;
        }
        // final LayerNorm (eps 1e-6) folded into the classifier     nrtr_decoder.py:77,111 + :78
        rc = tpspp_linear_ln_fwd(x, C, N, 1e-6f, c.w_cls, c.cls_colsum, c.num_out, c.b_cls, 0, nullptr, 0, c.W.logits, c.stream);
        if (rc) return rc;
        hipLaunchKernelGGL(dec_classify_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c.st, c.W.logits, c.num_out,
                           N, s, c.L, c.greedy, c.out, c.W.tokens, c.Lt, 0);
    }
    return TPSPP_OK;
}

int launch_attn_enc(const float* qkv, int N, int C, int T, const int* valid_len, float* out, hipStream_t st)
{
    const int H = C / kDK;
    const size_t M = (size_t)N * T;
    const size_t lds = (size_t)2 * T * kKRow * sizeof(float);
    static bool attr_done[tpspp::kMaxDevices] = {};
    if (tpspp::first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_enc_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipGetLastError();
    }
    if (T <= 128) {                                          // matrix-core kernel: a wavefront per 32 queries
        const int nj = (T + 31) / 32;
        const long waves = (long)N * H * nj;
        const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
        switch (nj) {
        case 1: hipLaunchKernelGGL(attn_enc_mfma_kernel<1>, grid, block, 0, st, qkv, C, (int)M, T, valid_len, out); break;
        case 2: hipLaunchKernelGGL(attn_enc_mfma_kernel<2>, grid, block, 0, st, qkv, C, (int)M, T, valid_len, out); break;
        case 3: hipLaunchKernelGGL(attn_enc_mfma_kernel<3>, grid, block, 0, st, qkv, C, (int)M, T, valid_len, out); break;
        default: hipLaunchKernelGGL(attn_enc_mfma_kernel<4>, grid, block, 0, st, qkv, C, (int)M, T, valid_len, out); break;
        }
        return tpspp::check_launch("attn_enc_mfma_kernel");
    }
    const int threads = kWave * ((T + kWave - 1) / kWave < 4 ? (T + kWave - 1) / kWave : 4);
    const dim3 grid((unsigned)((T + threads - 1) / threads), (unsigned)H, (unsigned)N);
    hipLaunchKernelGGL(attn_enc_kernel, grid, dim3(threads), lds, st, qkv, C, (int)M, T, valid_len, out);
    return tpspp::check_launch("attn_enc_kernel");
}

}  // namespace

TPSPP_EXPORT int tpspp_head_set_trace(long long* device_buf)
{
    g_head_trace = device_buf;
    return TPSPP_OK;
}

TPSPP_EXPORT int tpspp_lab_occupy(int workgroups, int lds_bytes, int milliseconds, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(workgroups > 0 && workgroups <= 4096 && lds_bytes >= 0 && lds_bytes <= 160 * 1024 && milliseconds > 0 && milliseconds <= 2000,
                  "tpspp_lab_occupy: workgroups in [1, 4096], lds_bytes in [0, 160 KB], milliseconds in [1, 2000]");
    static bool attr_done[tpspp::kMaxDevices] = {};
    if (tpspp::first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&lab_occupy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(lab_occupy_kernel, dim3((unsigned)workgroups), dim3(64), (size_t)lds_bytes, tpspp::as_stream(stream),
                       (long long)milliseconds * 100000, (int*)nullptr);
    return tpspp::check_launch("tpspp_lab_occupy");
}

TPSPP_EXPORT size_t tpspp_nrtr_encoder_workspace(int N, int C, int T, int d_inner)
{
    if (N <= 0 || C <= 0 || T <= 0 || d_inner <= 0) return 0;
    EncWorkspace W;
    W.layout(nullptr, N, C, T, d_inner);
    return W.bytes;
}

TPSPP_EXPORT size_t tpspp_nrtr_decoder_workspace(int N, int C, int T, int d_inner, int n_layers, int max_seq_len,
                                                 int num_out)
{
    if (N <= 0 || C <= 0 || T <= 0 || d_inner <= 0 || n_layers <= 0 || max_seq_len <= 0 || num_out <= 0) return 0;
    DecWorkspace W;
    W.layout(nullptr, N, C, T, d_inner, n_layers, max_seq_len, num_out);
    return W.bytes;
}

TPSPP_EXPORT int tpspp_transpose2d(const float* in, int rows, int cols, float* out, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(in && out && rows > 0 && cols > 0, "tpspp_transpose2d: bad argument");
    const dim3 grid((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32));
    TPSPP_REQUIRE(grid.y <= 65535, "tpspp_transpose2d: too many rows");
    hipLaunchKernelGGL(transpose2d_kernel, grid, dim3(256), 0, tpspp::as_stream(stream), in, rows, cols, out);
    return tpspp::check_launch("tpspp_transpose2d");
}

TPSPP_EXPORT int tpspp_layernorm_cm_fwd(const float* x, const float* gamma, const float* beta, int C, int M,
                                        float eps, float* y, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(x && gamma && beta && y && C > 0 && M > 0, "tpspp_layernorm_cm_fwd: bad argument");
    TPSPP_REQUIRE(C <= 1024, "tpspp_layernorm_cm_fwd: at most 1024 features");
    const dim3 grid((unsigned)((M + 15) / 16)), block(256);
    hipStream_t st = tpspp::as_stream(stream);
    if (C <= 128)      hipLaunchKernelGGL(layernorm_cm_kernel<8>, grid, block, 0, st, x, gamma, beta, C, M, eps, y);
    else if (C <= 512) hipLaunchKernelGGL(layernorm_cm_kernel<32>, grid, block, 0, st, x, gamma, beta, C, M, eps, y);
    else               hipLaunchKernelGGL(layernorm_cm_kernel<64>, grid, block, 0, st, x, gamma, beta, C, M, eps, y);
    return tpspp::check_launch("tpspp_layernorm_cm_fwd");
}

TPSPP_EXPORT int tpspp_attn_enc_fwd(const float* qkv, int N, int C, int T, const int* valid_len, float* out,
                                    tpspp_stream_t stream)
{
    TPSPP_REQUIRE(qkv && out && N > 0 && T > 0 && C > 0 && C % kDK == 0, "tpspp_attn_enc_fwd: bad argument (C must be a multiple of 64)");
    TPSPP_REQUIRE(T <= 256, "tpspp_attn_enc_fwd: at most 256 tokens per image");
    TPSPP_REQUIRE(N <= 65535 && (size_t)N * T < (1u << 31), "tpspp_attn_enc_fwd: batch too large");
    return launch_attn_enc(qkv, N, C, T, valid_len, out, tpspp::as_stream(stream));
}

TPSPP_EXPORT int tpspp_nrtr_encoder_fwd(const float* feat, int N, int C, int T, int d_inner, int n_layers,
                                        const float* const* layer_ptrs, const float* ln_g, const float* ln_b,
                                        const int* valid_len, void* workspace, size_t workspace_bytes,
                                        float* out_cm, float* out_ntc, int flags, tpspp_stream_t stream)
{
    const int x3 = (flags & TPSPP_HEAD_BF16X3) ? 1 : 0;
    const int b16 = (flags & (TPSPP_HEAD_BF16 | TPSPP_HEAD_BF16X3)) ? 1 : 0;
    TPSPP_REQUIRE(feat && layer_ptrs && ln_g && ln_b && workspace && (out_cm || out_ntc),
                  "tpspp_nrtr_encoder_fwd: null pointer");
    TPSPP_REQUIRE(N > 0 && T > 0 && n_layers > 0 && d_inner > 0 && C > 0 && C % kDK == 0,
                  "tpspp_nrtr_encoder_fwd: bad sizes (d_model must be a multiple of 64 = n_head * 64)");
    TPSPP_REQUIRE(T <= 256, "tpspp_nrtr_encoder_fwd: at most 256 tokens per image");
    TPSPP_REQUIRE(N <= 65535 && (size_t)N * T * 3 * C < ((size_t)1 << 40), "tpspp_nrtr_encoder_fwd: batch too large");
    EncWorkspace W;
    W.layout(workspace, N, C, T, d_inner);
    TPSPP_REQUIRE(workspace_bytes >= W.bytes, "tpspp_nrtr_encoder_fwd: workspace too small (%zu < %zu)", workspace_bytes,
                  W.bytes);
    for (int l = 0; l < n_layers; ++l) {
        const float* const* w = layer_ptrs + (size_t)l * E_COUNT;
        TPSPP_REQUIRE(w[E_LN1G] && w[E_LN1B] && w[E_WQKV] && w[E_WFC] && w[E_LN2G] && w[E_LN2B] && w[E_W1] && w[E_W2],
                      "tpspp_nrtr_encoder_fwd: layer %d has a null weight", l);
    }
    hipStream_t st = tpspp::as_stream(stream);
    const int M = N * T;
    float *x = W.x, *y = W.y, *a = W.a;
    {
        const size_t total = (size_t)N * C * T;
        const unsigned blocks = (unsigned)((total + 255) / 256 < 65535 * 16 ? (total + 255) / 256 : 65535 * 16);
        hipLaunchKernelGGL(nct_to_cm_kernel, dim3(blocks), dim3(256), 0, st, feat, N, C, T, x);
    }
    Gemm g{st, 0, b16, x3};
    int rc = 0;
    for (int l = 0; l < n_layers && !rc && !g.rc; ++l) {
        const float* const* w = layer_ptrs + (size_t)l * E_COUNT;
        // x = x + fc(attn(LN1(x)))                                   transformer_layers.py:67-70
        rc = tpspp_layernorm_cm_fwd(x, w[E_LN1G], w[E_LN1B], C, M, 1e-5f, y, stream);
        if (rc) break;
        g.proj(w[E_WQKV], w[E_BQKV], y, C, 3 * C, M, W.qkv, 0, nullptr);
        if (g.rc) break;
        rc = launch_attn_enc(W.qkv, N, C, T, valid_len, a, st);
        if (rc) break;
        g.proj(w[E_WFC], w[E_BFC], a, C, C, M, y, 0, x);              // y = x + fc(a)
        // x = y + w2(gelu(w1(LN2(y))))                                transformer_layers.py:72-75
        rc = tpspp_layernorm_cm_fwd(y, w[E_LN2G], w[E_LN2B], C, M, 1e-5f, a, stream);
        if (rc) break;
        g.proj(w[E_W1], w[E_B1], a, C, d_inner, M, W.hid, 2, nullptr);
        g.proj(w[E_W2], w[E_B2], W.hid, d_inner, C, M, x, 0, y);
    }
    if (rc) return rc;
    if (g.rc) return g.rc;
    float* fin = out_cm ? out_cm : y;
    rc = tpspp_layernorm_cm_fwd(x, ln_g, ln_b, C, M, 1e-5f, fin, stream);    // nrtr_encoder.py:85
    if (rc) return rc;
    if (out_ntc) return tpspp_transpose2d(fin, C, M, out_ntc, stream);        // (C, N*T) -> (N, T, C)
    return TPSPP_OK;
}

TPSPP_EXPORT int tpspp_nrtr_decoder_route(int C, int T, int d_inner, int n_layers, const float* const* layer_ptrs,
                                          int layer_ptrs_len, int num_out, int flags)
{
    TPSPP_REQUIRE(n_layers > 0 && layer_ptrs_len == n_layers * D_COUNT + 1,
                  "tpspp_nrtr_decoder_route: layer_ptrs_len must be n_layers * %d + 1", D_COUNT);
    TPSPP_REQUIRE(layer_ptrs && T > 0 && d_inner > 0 && C > 0 && C % kDK == 0 && num_out > 0,
                  "tpspp_nrtr_decoder_route: bad argument (d_model must be a multiple of 64)");
    const DecRoute R = dec_route(C, T, d_inner, n_layers, num_out, flags, dec_table_arranged(layer_ptrs, n_layers));
    return R.pipeline | (R.kv16 ? 4 : 0) | (R.gemm_f32 ? 8 : 0) | (R.cross2 ? 16 : 0) | ((R.persist + 1) << 8);
}

TPSPP_EXPORT int tpspp_nrtr_decoder_fwd(const float* enc_cm, int N, int C, int T, int d_inner, int n_layers,
                                        const float* const* layer_ptrs, int layer_ptrs_len,
                                        const float* emb, const float* pos_table, int n_position,
                                        const float* w_cls, const float* cls_colsum, const float* b_cls, int num_out,
                                        int max_seq_len,
                                        int start_idx, int padding_idx, const int* valid_len,
                                        const int* forced_tokens, void* workspace, size_t workspace_bytes,
                                        float* out, int* tokens_out, int* status_out, int flags, tpspp_stream_t stream)
{
    // ---- arguments
    TPSPP_REQUIRE(n_layers > 0 && layer_ptrs_len == n_layers * D_COUNT + 1,
                  "tpspp_nrtr_decoder_fwd: layer_ptrs_len must be n_layers * %d + 1 (24 pointers per layer, then the "
                  "arranged classifier)", D_COUNT);
    TPSPP_REQUIRE(enc_cm && layer_ptrs && emb && pos_table && w_cls && cls_colsum && workspace && out,
                  "tpspp_nrtr_decoder_fwd: null pointer");
    TPSPP_REQUIRE(N > 0 && T > 0 && n_layers > 0 && d_inner > 0 && C > 0 && C % kDK == 0 && num_out > 0,
                  "tpspp_nrtr_decoder_fwd: bad sizes (d_model must be a multiple of 64 = n_head * 64)");
    TPSPP_REQUIRE(T <= 256, "tpspp_nrtr_decoder_fwd: at most 256 encoder tokens per image");
    TPSPP_REQUIRE(max_seq_len >= 1 && max_seq_len <= kWave, "tpspp_nrtr_decoder_fwd: max_seq_len must be in [1, 64]");
    TPSPP_REQUIRE(n_position >= max_seq_len, "tpspp_nrtr_decoder_fwd: position table shorter than max_seq_len");
    // ---- layout
    DecCtx c;
    c.W.layout(workspace, N, C, T, d_inner, n_layers, max_seq_len, num_out);
    TPSPP_REQUIRE(workspace_bytes >= c.W.bytes, "tpspp_nrtr_decoder_fwd: workspace too small");
    TPSPP_REQUIRE(n_layers <= 64, "tpspp_nrtr_decoder_fwd: at most 64 layers");
    for (int l = 0; l < n_layers; ++l) {
        const float* const* w = layer_ptrs + (size_t)l * D_COUNT;
        TPSPP_REQUIRE(w[D_QKV_W] && w[D_QKV_CS] && w[D_WFC] && w[D_Q_W] && w[D_Q_CS] && w[D_WK] && w[D_WV] && w[D_WFC2] &&
                          w[D_W1_W] && w[D_W1_CS] && w[D_W2],
                      "tpspp_nrtr_decoder_fwd: layer %d has a null weight", l);
    }
    // ---- route
    c.R = dec_route(C, T, d_inner, n_layers, num_out, flags, dec_table_arranged(layer_ptrs, n_layers));
    // ---- what the parts below share
    c.st = tpspp::as_stream(stream); c.stream = stream;
    c.N = N; c.C = C; c.T = T; c.H = C / kDK; c.d_inner = d_inner; c.n_layers = n_layers; c.num_out = num_out;
    c.L = max_seq_len; c.Lt = max_seq_len + 1;
    c.enc_cm = enc_cm; c.layer_ptrs = layer_ptrs; c.cls_x = layer_ptrs[(size_t)n_layers * D_COUNT];
    c.emb = emb; c.pos_table = pos_table; c.w_cls = w_cls; c.cls_colsum = cls_colsum; c.b_cls = b_cls;
    c.padding_idx = padding_idx; c.greedy = forced_tokens ? 0 : 1; c.valid_len = valid_len; c.out = out;
    // ---- run
    if (int rc = TPSPP_HEAD_KV(c, project_encoder_kv)) return rc;
    hipLaunchKernelGGL(dec_init_tokens_kernel, dim3((unsigned)((N * c.Lt + 255) / 256)), dim3(256), 0, c.st, c.W.tokens, N,
                       c.Lt, start_idx, padding_idx, forced_tokens, c.L);
    // a persistent-eligible route: the device and the environment have the last word
    PersistEnv env{};
    int dev = 0, groups = 0;
    if (c.R.pipeline == kDecPersistent) {
        env = read_persist_env();
        groups = persist_groups_now(c, env, dev);
    }
    if (groups > 0) return decode_persistent(c, env, dev, groups, tokens_out, status_out);
    if (status_out && hipMemsetAsync(status_out, 0, sizeof(int), c.st) != hipSuccess)
        return tpspp::check_launch("tpspp_nrtr_decoder_fwd(status)");
    if (int rc = c.R.pipeline == kDecPlain ? TPSPP_HEAD_KV(c, decode_steps_plain) : TPSPP_HEAD_KV(c, decode_steps_arranged))
        return rc;
    if (tokens_out)
        (void)hipMemcpyAsync(tokens_out, c.W.tokens, (size_t)N * c.Lt * sizeof(int), hipMemcpyDeviceToDevice, c.st);
    return tpspp::check_launch("tpspp_nrtr_decoder_fwd");
}

TPSPP_EXPORT int tpspp_attn_tensor2idx_fwd(const float* scores, int N, int L, int C, int end_idx, int padding_idx,
                                           int* idx_out, float* val_out, tpspp_stream_t stream)
{
    TPSPP_REQUIRE(scores && idx_out && val_out && N > 0 && L > 0 && C > 0, "tpspp_attn_tensor2idx_fwd: bad argument");
    TPSPP_REQUIRE((size_t)N * L * C < ((size_t)1 << 40) && N <= (1 << 30), "tpspp_attn_tensor2idx_fwd: batch too large");
    hipLaunchKernelGGL(attn_tensor2idx_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, tpspp::as_stream(stream), scores, N, L, C,
                       end_idx, padding_idx, idx_out, val_out);
    return tpspp::check_launch("tpspp_attn_tensor2idx_fwd");
}
