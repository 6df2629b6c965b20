// The optimiser stage of a training iteration (include/tpspp_train_opt.h): multi-tensor Adam / AdamW, the gradient norm
// with its clipping coefficient, and the zeroing of all gradients, each one launch over every parameter tensor.
//
// replaces: the per-tensor loops of torch.optim.Adam / AdamW (_single_tensor_adam), torch.nn.utils.clip_grad_norm_ and
// the clip-then-step of mmcv's OptimizerHook.
//
//   * One workgroup per row of the chunk map; the tensor's addresses, its element count and its scalar row are read from
//     device memory (wave-uniform loads).  Thread i owns the elements 4i .. 4i+3 of every slice of 4 * blockDim elements: as
//     one 128-bit access per array where all four addresses are 16-byte aligned, element by element otherwise (a view
//     at an odd offset, the last one to three elements of a tensor).  The ownership is the same on both paths, so the
//     per-thread sums of mt_sumsq_kernel do not depend on the path.
//   * A streaming job with no reuse: 16 B read per array and thread per trip, no LDS in the update, few registers, so
//     many workgroups per CU keep enough loads in flight.
//   * No atomics: a partial sum per chunk (thread sums ascending, a fixed butterfly per wavefront, wavefronts ascending),
//     then mt_norm_finish_kernel adds the partials in index order in fp64.
//   * Built with -ffp-contract=off: the only fused products are the fmaf() calls below, the ones the header names.
#include "tpspp_common.h"
#include "tpspp_train_opt.h"

#include <math.h>
#include <stdint.h>

namespace {

constexpr int kMaxThreads = 1024;
constexpr int kMaxChunk = 1 << 20;
constexpr int kFinishThreads = 256;

struct Chunk {
    long long ti, first, count;
    int n;              // elements of this chunk, 0: nothing to do
};

__device__ inline Chunk chunk_of(const long long* table, int n_tensors, const long long* chunk_map, int chunk)
{
    Chunk c;
    c.ti = chunk_map[2 * (long long)blockIdx.x];
    c.first = chunk_map[2 * (long long)blockIdx.x + 1];
    c.count = 0;
    c.n = 0;
    if (c.ti < 0 || c.ti >= n_tensors) return c;
    c.count = table[5 * c.ti + 4];
    if (c.first < 0 || c.first >= c.count) return c;
    const long long left = c.count - c.first;
    c.n = left < chunk ? (int)left : chunk;
    return c;
}

// Addresses come out of the table as integers: name the global address space, or every access would be a flat one.
typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gfloat4;

__device__ inline gfloat* at(long long address, long long first) { return reinterpret_cast<gfloat*>(address) + first; }
__device__ inline bool aligned16(const gfloat* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
__device__ inline f32x4 load128(const gfloat* a) { return *reinterpret_cast<const gfloat4*>(a); }
__device__ inline void store128(gfloat* a, f32x4 x) { *reinterpret_cast<gfloat4*>(a) = x; }

struct AdamArgs {
    float step_size, bc2_sqrt, wd, decay, beta2, omb1, omb2, eps, coef;
    bool clip, l2, adamw;
};

__device__ inline void adam1(const AdamArgs& a, float& p, float g, float& m, float& v)
{
    if (a.clip) g = a.coef * g;
    if (a.l2) g = fmaf(a.wd, p, g);
    if (a.adamw) p = p * a.decay;
    m = fmaf(a.omb1, g - m, m);
    v = fmaf(a.omb2 * g, g, a.beta2 * v);
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = fmaf(-a.step_size, m / denom, p);
}

__global__ void __launch_bounds__(kMaxThreads)
mt_adam_kernel(const long long* table, const float* scalars, int n_tensors, const long long* chunk_map, int chunk,
               float beta2, float omb1, float omb2, float eps, int mode, const float* coef)
{
    const Chunk c = chunk_of(table, n_tensors, chunk_map, chunk);
    if (c.n == 0) return;
    const long long* row = table + 5 * c.ti;
    gfloat* p = at(row[0], c.first);
    const gfloat* g = at(row[1], c.first);
    gfloat* m = at(row[2], c.first);
    gfloat* v = at(row[3], c.first);
    AdamArgs a;
    a.step_size = scalars[4 * c.ti], a.bc2_sqrt = scalars[4 * c.ti + 1], a.wd = scalars[4 * c.ti + 2];
    a.decay = scalars[4 * c.ti + 3];
    a.beta2 = beta2, a.omb1 = omb1, a.omb2 = omb2, a.eps = eps;
    a.clip = coef != nullptr;
    a.coef = a.clip ? coef[0] : 1.f;
    a.adamw = mode == TPSPP_OPT_ADAMW;
    a.l2 = !a.adamw && a.wd != 0.f;
    const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v);

    for (int i = 4 * (int)threadIdx.x; i < c.n; i += 4 * (int)blockDim.x) {
        if (vec && c.n - i >= 4) {
            const f32x4 p4 = load128(p + i), m4 = load128(m + i), v4 = load128(v + i), g4 = load128(g + i);
            float pp[4] = {p4.x, p4.y, p4.z, p4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
            const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) adam1(a, pp[j], gg[j], mm[j], vv[j]);
            store128(p + i, f32x4{pp[0], pp[1], pp[2], pp[3]});
            store128(m + i, f32x4{mm[0], mm[1], mm[2], mm[3]});
            store128(v + i, f32x4{vv[0], vv[1], vv[2], vv[3]});
        } else {
            const int end = c.n - i < 4 ? c.n : i + 4;
            for (int e = i; e < end; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam1(a, pe, g[e], me, ve);
                p[e] = pe, m[e] = me, v[e] = ve;
            }
        }
    }
}

__global__ void __launch_bounds__(kMaxThreads)
mt_sumsq_kernel(const long long* table, int n_tensors, const long long* chunk_map, int chunk, float* partials)
{
    __shared__ float wave_sum[kMaxThreads / 64];
    const Chunk c = chunk_of(table, n_tensors, chunk_map, chunk);      // uniform over the workgroup
    float acc = 0.f;
    if (c.n != 0) {
        const gfloat* g = at(table[5 * c.ti + 1], c.first);
        const bool vec = aligned16(g);
        for (int i = 4 * (int)threadIdx.x; i < c.n; i += 4 * (int)blockDim.x) {
            if (vec && c.n - i >= 4) {
                const f32x4 gg = load128(g + i);
                acc = fmaf(gg.x, gg.x, acc);
                acc = fmaf(gg.y, gg.y, acc);
                acc = fmaf(gg.z, gg.z, acc);
                acc = fmaf(gg.w, gg.w, acc);
            } else {
                const int end = c.n - i < 4 ? c.n : i + 4;
                for (int e = i; e < end; ++e) acc = fmaf(g[e], g[e], acc);
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = wave_sum[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) s += wave_sum[w];
        partials[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kMaxThreads)
mt_zero_kernel(const long long* table, int n_tensors, const long long* chunk_map, int chunk)
{
    const Chunk c = chunk_of(table, n_tensors, chunk_map, chunk);
    if (c.n == 0) return;
    gfloat* g = at(table[5 * c.ti + 1], c.first);
    const bool vec = aligned16(g);
    for (int i = 4 * (int)threadIdx.x; i < c.n; i += 4 * (int)blockDim.x) {
        if (vec && c.n - i >= 4) {
            store128(g + i, f32x4{0.f, 0.f, 0.f, 0.f});
        } else {
            const int end = c.n - i < 4 ? c.n : i + 4;
            for (int e = i; e < end; ++e) g[e] = 0.f;
        }
    }
}

__global__ void __launch_bounds__(kFinishThreads)
mt_norm_finish_kernel(const float* partials, int n_chunks, float max_norm, float* out)
{
    __shared__ double part[kFinishThreads];
    const int per = (n_chunks + kFinishThreads - 1) / kFinishThreads;
    const int lo = (int)threadIdx.x * per;
    const int hi = lo + per < n_chunks ? lo + per : n_chunks;
    double s = 0.0;
    for (int i = lo; i < hi; ++i) s += (double)partials[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < kFinishThreads; ++i) total += part[i];
        const float norm = (float)sqrt(total);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;                   // NaN stays NaN, as torch.clamp(max=1) leaves it
        out[2] = isfinite(norm) ? 0.f : 1.f;
    }
}

int check_map(const char* who, const void* table, int n_tensors, const void* chunk_map, int n_chunks, int chunk, int threads)
{
    TPSPP_REQUIRE(table && chunk_map, "%s: null pointer", who);
    TPSPP_REQUIRE(n_tensors > 0 && n_chunks > 0, "%s: bad sizes (n_tensors %d, n_chunks %d must be positive)", who, n_tensors,
                  n_chunks);
    TPSPP_REQUIRE(chunk > 0 && chunk % 4 == 0 && chunk <= kMaxChunk,
                  "%s: chunk %d must be a positive multiple of 4 (the vector width), at most %d", who, chunk, kMaxChunk);
    TPSPP_REQUIRE(threads == 64 || threads == 128 || threads == 256 || threads == 512 || threads == 1024,
                  "%s: threads %d must be 64, 128, 256, 512 or 1024", who, threads);
    return TPSPP_OK;
}

}  // namespace

TPSPP_EXPORT int tpspp_mt_adam(const long long* table, const float* scalars, int n_tensors, const long long* chunk_map,
                               int n_chunks, int chunk, int threads, double beta1, double beta2, double eps, int mode,
                               const float* coef, tpspp_stream_t stream)
{
    const char* who = "tpspp_mt_adam";
    if (int rc = check_map(who, table, n_tensors, chunk_map, n_chunks, chunk, threads)) return rc;
    TPSPP_REQUIRE(scalars, "%s: null pointer", who);
    TPSPP_REQUIRE(mode == TPSPP_OPT_ADAM || mode == TPSPP_OPT_ADAMW, "%s: mode %d is neither Adam (0) nor AdamW (1)", who, mode);
    TPSPP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: betas must lie in [0, 1)", who);
    TPSPP_REQUIRE(eps >= 0.0 && isfinite(eps), "%s: eps must be finite and not negative", who);
    // the betas arrive in double: 1 - (float)0.999 would be off by 1.3e-5 of itself, which sqrt(v) carries into the step
    hipLaunchKernelGGL(mt_adam_kernel, dim3((unsigned)n_chunks), dim3((unsigned)threads), 0, tpspp::as_stream(stream), table,
                       scalars, n_tensors, chunk_map, chunk, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                       (float)eps, mode, coef);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_mt_sumsq(const long long* table, int n_tensors, const long long* chunk_map, int n_chunks, int chunk,
                                int threads, float* partials, size_t partial_floats, tpspp_stream_t stream)
{
    const char* who = "tpspp_mt_sumsq";
    if (int rc = check_map(who, table, n_tensors, chunk_map, n_chunks, chunk, threads)) return rc;
    TPSPP_REQUIRE(partials, "%s: null pointer", who);
    TPSPP_REQUIRE(partial_floats >= (size_t)n_chunks, "%s: workspace of %zu floats, %d needed", who, partial_floats, n_chunks);
    hipLaunchKernelGGL(mt_sumsq_kernel, dim3((unsigned)n_chunks), dim3((unsigned)threads), 0, tpspp::as_stream(stream), table,
                       n_tensors, chunk_map, chunk, partials);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_mt_norm_finish(const float* partials, int n_chunks, float max_norm, float* out, tpspp_stream_t stream)
{
    const char* who = "tpspp_mt_norm_finish";
    TPSPP_REQUIRE(partials && out, "%s: null pointer", who);
    TPSPP_REQUIRE(n_chunks > 0, "%s: bad sizes (n_chunks %d must be positive)", who, n_chunks);
    TPSPP_REQUIRE(max_norm > 0.f, "%s: max_norm must be positive", who);
    hipLaunchKernelGGL(mt_norm_finish_kernel, dim3(1), dim3(kFinishThreads), 0, tpspp::as_stream(stream), partials, n_chunks,
                       max_norm, out);
    return tpspp::check_launch(who);
}

TPSPP_EXPORT int tpspp_mt_zero(const long long* table, int n_tensors, const long long* chunk_map, int n_chunks, int chunk,
                               int threads, tpspp_stream_t stream)
{
    const char* who = "tpspp_mt_zero";
    if (int rc = check_map(who, table, n_tensors, chunk_map, n_chunks, chunk, threads)) return rc;
    hipLaunchKernelGGL(mt_zero_kernel, dim3((unsigned)n_chunks), dim3((unsigned)threads), 0, tpspp::as_stream(stream), table,
                       n_tensors, chunk_map, chunk);
    return tpspp::check_launch(who);
}
