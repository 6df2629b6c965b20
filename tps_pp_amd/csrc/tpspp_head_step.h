// Device code of the recogniser head, second part: the decoder step -- embedding, attention against the caches and the
// encoder, classifier epilogue, the step GEMMs (with the persistent step kernel, tpspp_head_persist.h, between them) -- and
// the device-side AttnConvertor.tensor2idx.  Included by tpspp_head.hip inside its anonymous namespace, behind
// tpspp_head_kernels.h.
#pragma once

// ---- decoder, one step: embedding + position table ----------------------------------------------------
// x[c][b] = emb[tokens[b][step]][c] + pos[step][c]      (nrtr_decoder.py:96-98, no scaling)
// tm: x is token-major (Nb, C) instead of channel-major (C, Nb) (the split-K step GEMM's layout)
__global__ void __launch_bounds__(256)
dec_embed_kernel(const float* __restrict__ emb, const float* __restrict__ pos, const int* __restrict__ tokens,
                 int Lt, int step, int C, int Nb, float* __restrict__ x, int tm)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * Nb) return;
    const int c = tm ? i % C : i / Nb, b = tm ? i / C : i - c * Nb;
    const int tok = tokens[(size_t)b * Lt + step];
    x[i] = emb[(size_t)tok * C + c] + pos[(size_t)step * C + c];
}

// ---- decoder, one step: attention against the caches / the encoder, 16-byte loads -----------------------------------
// qkv_t (Nb, 3C) / q_t (Nb, C) TOKEN-major (this step's projections); one wavefront per (image, head).
// Self-attention (nrtr_decoder.py:100-102): key p is valid iff p <= step and tokens[b][p] != <PAD>; the new position is
// used from registers, so nothing written by the kernel is read back by it.  Cross-attention (nrtr_decoder.py:115-129):
// keys >= valid_len[b] are masked.  KV = float, or unsigned short: bf16 caches / encoder keys and values
// (TPSPP_HEAD_BF16: the encoder K/V are the only HBM-bound operand of a step; the position being decoded is used from its
// fp32 registers, earlier positions as they were rounded when written; scores, softmax, weighted sum in fp32).
// Rounds 1-2 gave a lane one 4-byte element per load (a key row per lane, a value row per wavefront): 128 load
// instructions of 256 bytes per (image, head), and the vector-memory unit takes 16 cycles per instruction whatever its
// width -- the cross-attention's 134 MB per layer-step moved at 4 TB/s.  Here keys AND values are token-major
// ((tokens, C) rows, a head's 64 features contiguous), a lane takes 16 bytes (EPL = 4 fp32 or 8 bf16 features) of a
// token, GS = 64 / EPL lanes share a token and a load instruction covers 64 / GS tokens x one contiguous head row:
// 4x (8x) fewer instructions for the same bytes.  Scores: per-lane partial dot products, summed inside the GS-lane
// group on the DPP path (quad swaps, half-row / row mirror); values: per-lane partial sums over the lane's tokens,
// summed across the groups with a few lane exchanges at the very end.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int GS> __device__ __forceinline__ float group_sum(float v)      // every lane of a GS-lane group: the group's sum
{
    v = dpp_add<0xB1>(v);                      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);                      // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);                     // row_half_mirror: 8 lanes
    if (GS == 16) v = dpp_add<0x140>(v);       // row_mirror: 16 lanes
    return v;
}
template <int GS> __device__ __forceinline__ float across_groups_sum(float v)   // sum over the 64 / GS groups (same lane of each)
{
    if (GS == 8) v += __shfl_xor(v, 8, kWave);
    v += __shfl_xor(v, 16, kWave);
    v += __shfl_xor(v, 32, kWave);
    return v;
}
template <int GS> __device__ __forceinline__ float across_groups_max(float v)
{
    if (GS == 8) v = fmaxf(v, __shfl_xor(v, 8, kWave));
    v = fmaxf(v, __shfl_xor(v, 16, kWave));
    v = fmaxf(v, __shfl_xor(v, 32, kWave));
    return v;
}

// ---- system-scope (sc0 sc1) accesses for data exchanged between workgroups INSIDE one launch (the persistent decoder
// step, tpspp_head_persist.h): they bypass the CU's L1 and the XCD's L2, so a value written by another CU -- maybe on
// another XCD -- is never served from a stale line (MI355X_MICROARCH.md, "sc0 sc1 stores and loads both sides").  The loads
// are inline asm, invisible to the compiler's wait-count tracking: every use must sit behind a wait_sys() that names the
// loaded registers.
typedef float hf32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hf32x4 ld16_sys(const float* p)
{
    hf32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ void st16_sys(float* p, hf32x4 v)
{
    // (s_nop: the VMEM store-data hazard is invisible to the compiler inside inline asm, as in tpspp_warp_pair.h)
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// `plain` (the persistent step kernel, when the 16 workgroups of a cluster were verified to sit on ONE XCD): an ordinary store --
// the line stays in that XCD's L2, where the cluster's sc0 sc1 loads (which bypass L1 only) find it at the L2's latency; a
// write-through store drops the line and the same reader fetches it over the fabric (MI355X_MICROARCH.md, "stores of each flavour").
__device__ __forceinline__ void st16_x(float* p, hf32x4 v, bool plain)
{
    if (plain) asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void wait_sys(hf32x4& a) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(a)::"memory"); }
__device__ __forceinline__ void wait_sys(hf32x4& a, hf32x4& b, hf32x4& c)
{
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c)::"memory");
}
// the same load as two 8-byte system-scope atomic loads: VISIBLE to the compiler (it tracks their wait count itself and may
// schedule them among other loads) -- for small operands whose latency should overlap other requests
__device__ __forceinline__ hf32x4 ld16_sys_v(const float* p)
{
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return hf32x4{__builtin_bit_cast(float, (unsigned)lo), __builtin_bit_cast(float, (unsigned)(lo >> 32)),
                  __builtin_bit_cast(float, (unsigned)hi), __builtin_bit_cast(float, (unsigned)(hi >> 32))};
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

struct NoPre { __device__ __forceinline__ bool operator()() const { return true; } };   // (see self_attend's `pre`)

template <typename KV> struct Wide;
template <> struct Wide<float> {
    static constexpr int EPL = 4;
    typedef float4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float (&f)[4]) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
    static __device__ __forceinline__ raw pack(const float (&f)[4]) { return make_float4(f[0], f[1], f[2], f[3]); }
};
template <> struct Wide<unsigned short> {
    static constexpr int EPL = 8;
    typedef uint4 raw;
    static __device__ __forceinline__ void unpack(const raw& r, float (&f)[8])
    {
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[2 * i] = __builtin_bit_cast(float, w[i] << 16); f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u); }
    }
    static __device__ __forceinline__ raw pack(const float (&f)[8])
    {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                      // round to nearest even, as kvc_store
            unsigned a = __builtin_bit_cast(unsigned, f[2 * i]), b = __builtin_bit_cast(unsigned, f[2 * i + 1]);
            a += 0x7fffu + ((a >> 16) & 1u); b += 0x7fffu + ((b >> 16) & 1u);
            w[i] = (a >> 16) | (b & 0xffff0000u);
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
};

// cross-attention of one (image b, head h) by one wavefront: q (this lane's EPL features, already scaled), Kx_t / Vx_t
// (Nb*T, C) token-major, out (Nb, C) token-major (or channel-major).
// MAXJJ: 64-token groups the code is built for (T <= 64 MAXJJ; 1 saves 48 registers of score storage)
template <typename KV, bool SYS = false, int MAXJJ = 4>
__device__ __forceinline__ void cross_attend(const float (&q)[Wide<KV>::EPL], const KV* __restrict__ Kx_t, const KV* __restrict__ Vx_t,
                                             int C, int Nb, int T, int nvalid, int b, int h, int lane, float* __restrict__ out,
                                             int out_cm, bool plain_st = false)
{
    typedef Wide<KV> Wd;
    constexpr int EPL = Wd::EPL, GS = kDK / EPL, TPI = kWave / GS, NP = kWave / TPI;   // tokens per instruction, pieces per 64 tokens
    const int grp = lane / GS, dl = lane % GS;             // this lane: tokens grp, grp + TPI, ...; features EPL dl ..
    const typename Wd::raw* kb = reinterpret_cast<const typename Wd::raw*>(Kx_t + ((size_t)b * T) * C + kDK * h + EPL * dl);
    const typename Wd::raw* vb = reinterpret_cast<const typename Wd::raw*>(Vx_t + ((size_t)b * T) * C + kDK * h + EPL * dl);
    const size_t rstride = (size_t)C / EPL;                // row pitch in raw pieces
    float sc[MAXJJ][NP];
    float mx = -INFINITY;
#pragma unroll
    for (int jj = 0; jj < MAXJJ; ++jj) {
#pragma unroll
        for (int i = 0; i < NP; ++i) sc[jj][i] = -INFINITY;
        if (jj * kWave < nvalid) {                         // wave-uniform
            typename Wd::raw kr[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) {                 // every key piece of these 64 tokens in flight together
                const int t = jj * kWave + TPI * i + grp;
                kr[i] = kb[(size_t)(t < T ? t : T - 1) * rstride];
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                float kf[EPL];
                Wd::unpack(kr[i], kf);
                float s = 0.0f;
#pragma unroll
                for (int e = 0; e < EPL; ++e) s = fmaf(q[e], kf[e], s);
                s = group_sum<GS>(s);
                const int t = jj * kWave + TPI * i + grp;
                sc[jj][i] = t < nvalid ? s : -INFINITY;
                mx = fmaxf(mx, sc[jj][i]);
            }
        }
    }
    mx = across_groups_max<GS>(mx);
    float l = 0.0f;
#pragma unroll
    for (int jj = 0; jj < MAXJJ; ++jj)
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            sc[jj][i] = sc[jj][i] == -INFINITY ? 0.0f : expf(sc[jj][i] - mx);
            l += sc[jj][i];
        }
    l = across_groups_sum<GS>(l);
    const float inv = 1.0f / l;
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int jj = 0; jj < MAXJJ; ++jj) {
        if (jj * kWave < nvalid) {
            typename Wd::raw vr[NP];
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int t = jj * kWave + TPI * i + grp;
                vr[i] = vb[(size_t)(t < T ? t : T - 1) * rstride];
            }
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                float vf[EPL];
                Wd::unpack(vr[i], vf);
                const float pw = sc[jj][i] * inv;          // 0 for masked tokens
#pragma unroll
                for (int e = 0; e < EPL; ++e) acc[e] = fmaf(pw, vf[e], acc[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = across_groups_sum<GS>(acc[e]);
    if (grp == 0) {
        if (out_cm) {                                      // channel-major (C, Nb): the exact-fp32 step GEMMs' operand layout
#pragma unroll
            for (int e = 0; e < EPL; ++e) out[(size_t)(kDK * h + EPL * dl + e) * Nb + b] = acc[e];
        } else {
            float* o = out + (size_t)b * C + kDK * h + EPL * dl;
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                if (SYS) st16_x(o + e, hf32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]}, plain_st);
                else *reinterpret_cast<float4*>(o + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
            }
        }
    }
}

// cross-attention of image b, heads h and h + 1, by one wavefront, T <= 64 encoder tokens: cross_attend's arithmetic per head
// (same fragments, same reduction order), every stage run for BOTH heads before the next one starts -- the keys of both heads
// are in flight together, then the values of both (8 wavefronts per CU must keep as many requests outstanding as the 16 of
// the launch form; in the launch form itself two heads per wavefront measured 22-23 us per launch against 28.6 with one).
// SYS: q via compiler-visible system-scope loads, output system-scope (the persistent step kernel).
template <typename KV, bool SYS, typename Pre = NoPre>
__device__ __forceinline__ bool cross_attend2(const float* __restrict__ qrow, const KV* __restrict__ Kx_t, const KV* __restrict__ Vx_t,
                                              int C, int T, int nvalid, int b, int h, int lane, float* __restrict__ out, Pre pre = Pre(), bool plain_st = false)
{
    typedef Wide<KV> Wd;
    constexpr int EPL = Wd::EPL, GS = kDK / EPL, TPI = kWave / GS, NP = kWave / TPI, NH = 2;
    const int grp = lane / GS, dl = lane % GS;
    const size_t rstride = (size_t)C / EPL;                // row pitch in raw pieces
    typename Wd::raw kr[NH][NP], vr[NH][NP];
    float q[NH][EPL], sc[NH][NP], inv[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        const typename Wd::raw* kb = reinterpret_cast<const typename Wd::raw*>(Kx_t + ((size_t)b * T) * C + kDK * (h + n) + EPL * dl);
#pragma unroll
        for (int i = 0; i < NP; ++i) {                     // every key piece of both heads in flight together
            const int t = TPI * i + grp;
            kr[n][i] = kb[(size_t)(t < T ? t : T - 1) * rstride];
        }
    }
    // (the keys do not depend on this step: they were requested in front of `pre`, the barrier behind which q is readable)
    if (!pre()) return false;
#pragma unroll
    for (int n = 0; n < NH; ++n) {
#pragma unroll
        for (int e = 0; e < EPL / 4; ++e) {
            const float* qp = qrow + kDK * (h + n) + EPL * dl + 4 * e;
            const hf32x4 rq = SYS ? ld16_sys_v(qp) : *reinterpret_cast<const hf32x4*>(qp);
#pragma unroll
            for (int i = 0; i < 4; ++i) q[n][4 * e + i] = rq[i] * 0.125f;
        }
    }
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            float kf[EPL];
            Wd::unpack(kr[n][i], kf);
            float s = 0.0f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) s = fmaf(q[n][e], kf[e], s);
            s = group_sum<GS>(s);
            const int t = TPI * i + grp;
            sc[n][i] = t < nvalid ? s : -INFINITY;
            mx = fmaxf(mx, sc[n][i]);
        }
        mx = across_groups_max<GS>(mx);
        float l = 0.0f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            sc[n][i] = sc[n][i] == -INFINITY ? 0.0f : expf(sc[n][i] - mx);
            l += sc[n][i];
        }
        l = across_groups_sum<GS>(l);
        inv[n] = 1.0f / l;
    }
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        const typename Wd::raw* vb = reinterpret_cast<const typename Wd::raw*>(Vx_t + ((size_t)b * T) * C + kDK * (h + n) + EPL * dl);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int t = TPI * i + grp;
            vr[n][i] = vb[(size_t)(t < T ? t : T - 1) * rstride];
        }
    }
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            float vf[EPL];
            Wd::unpack(vr[n][i], vf);
            const float pw = sc[n][i] * inv[n];            // 0 for masked tokens
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] = fmaf(pw, vf[e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = across_groups_sum<GS>(acc[e]);
        if (grp == 0) {
            float* o = out + (size_t)b * C + kDK * (h + n) + EPL * dl;
#pragma unroll
            for (int e = 0; e < EPL; e += 4) {
                if (SYS) st16_x(o + e, hf32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]}, plain_st);
                else *reinterpret_cast<float4*>(o + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
            }
        }
    }
    return true;
}


// cross-attention: q_t (Nb, C), Kx_t / Vx_t (Nb*T, C) token-major, out (Nb, C) token-major.  One wavefront per (image, head).
template <typename KV>
__global__ void __launch_bounds__(256)
attn_dec_cross_wide_kernel(const float* __restrict__ q_t, const KV* __restrict__ Kx_t, const KV* __restrict__ Vx_t,
                           int C, int Nb, int H, int T, const int* __restrict__ valid_len, float* __restrict__ out, int out_cm)
{
    constexpr int EPL = Wide<KV>::EPL, GS = kDK / EPL;
    const int lane = threadIdx.x & (kWave - 1);
    const int pair = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= Nb * H) return;
    const int b = pair / H, h = pair - b * H;
    const int dl = lane % GS;
    float q[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) q[e] = q_t[(size_t)b * C + kDK * h + EPL * dl + e] * 0.125f;
    int nvalid = valid_len ? valid_len[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    cross_attend<KV>(q, Kx_t, Vx_t, C, Nb, T, nvalid, b, h, lane, out, out_cm);
}

// two heads per wavefront (T <= 64, H even, token-major output): q_t rows at pitch `ldq`
template <typename KV>
__global__ void __launch_bounds__(256)
attn_dec_cross_wide2_kernel(const float* __restrict__ q_t, int ldq, const KV* __restrict__ Kx_t, const KV* __restrict__ Vx_t,
                            int C, int Nb, int H, int T, const int* __restrict__ valid_len, float* __restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int pair2 = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // (image, head pair)
    const int H2 = H >> 1;
    if (pair2 >= Nb * H2) return;
    const int b = pair2 / H2, h = 2 * (pair2 - b * H2);
    int nvalid = valid_len ? valid_len[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    cross_attend2<KV, false>(q_t + (size_t)b * ldq, Kx_t, Vx_t, C, T, nvalid, b, h, lane, out);
}


// masked self-attention against token-major caches Kc / Vc [image][head][position][64]; qkv_t (Nb, 3C); out (Nb, C).
// The new position's key / value are used from registers (fp32) and appended to the caches.
// NH consecutive heads h .. h + NH - 1 of image b by one wavefront (NH = 1: the launch-per-phase kernel; 2: the persistent
// step kernel, whose 8 wavefronts per CU need both heads' requests in flight together to keep the memory system as busy as
// the 16 wavefronts per CU of the launch form do -- every stage below runs over the NH heads before the next stage starts).
// SYS (the persistent step kernel): this step's q | k | v row and the output are exchanged with other workgroups of the same
// launch -- system-scope accesses; the caches belong to earlier / later launches and stay plain.
// `pre` (the persistent step kernel): called once the requests that do NOT depend on this step's projections are in flight --
// the cached keys / values and the token ids --; it is the cluster barrier behind which q | k | v become readable (false =
// barrier timeout: give up).
template <typename KV, bool SYS, int NH = 1, typename Pre = NoPre>
__device__ __forceinline__ bool self_attend(const float* __restrict__ qkv_t, int C, int Nb, int H, int step, int Lmax,
                                            KV* __restrict__ Kc, KV* __restrict__ Vc, const int* __restrict__ tokens, int Lt,
                                            int pad_idx, float* __restrict__ out, int out_cm, int b, int h, int lane, Pre pre = Pre(), bool plain_st = false)
{
    typedef Wide<KV> Wd;
    constexpr int EPL = Wd::EPL, GS = kDK / EPL, TPI = kWave / GS, NP = kWave / TPI;
    const int grp = lane / GS, dl = lane % GS;
    float q[NH][EPL], k[NH][EPL], v[NH][EPL];
    typename Wd::raw *kc[NH], *vc[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        const size_t bh = (size_t)b * H + h + n;
        kc[n] = reinterpret_cast<typename Wd::raw*>(Kc + bh * Lmax * kDK + EPL * dl);
        vc[n] = reinterpret_cast<typename Wd::raw*>(Vc + bh * Lmax * kDK + EPL * dl);
    }
    constexpr int rstride = GS;                            // a cached row is GS pieces

    // Every load of the wavefront is requested here, before the first use of any of them: the cached keys AND values of the
    // earlier positions (the values do not depend on the scores) and the positions' token ids (the <PAD> mask).  Round 4: the
    // ids used to be read inside the score loop, one 4-byte load and one s_waitcnt vmcnt(0) per piece, and the values behind
    // the softmax -- eleven dependent round trips to memory in a kernel that moves 5-20 KB per wavefront (9-13 us per launch,
    // 240 launches per batch); now three (four with fp32 caches).
    // (fp32 caches: keys + values together are 128 registers of loads in flight, 140 in all -- three wavefronts per SIMD
    // instead of four, i.e. a second, nearly empty round of the 4096 wavefronts: 16.7 us against 13.4; their values stay
    // behind the softmax.  bf16 caches: 123 registers, 9.2 -> 8.9 us.)
    constexpr bool kValuesEarly = sizeof(KV) == 2;
    float sc[NH][NP];
    typename Wd::raw kr[NH][NP], vr[NH][NP];
    int tk[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = TPI * i + grp;
        tk[i] = pad_idx;
        if (TPI * i <= step) {                                 // (uniform tests: whole pieces beyond `step` are skipped)
            const int* tp = tokens + (size_t)b * Lt + (p <= step ? p : 0);
            // (SYS: the previous step of the same launch wrote the newest id)
            tk[i] = SYS ? __hip_atomic_load(tp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : *tp;
        }
        if (TPI * i < step) {
#pragma unroll
            for (int n = 0; n < NH; ++n) {
                kr[n][i] = kc[n][(size_t)(p < step ? p : 0) * rstride];
                if (kValuesEarly) vr[n][i] = vc[n][(size_t)(p < step ? p : 0) * rstride];
            }
        }
    }
    if (!pre()) return false;
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        const float* base = qkv_t + (size_t)b * 3 * C + kDK * (h + n) + EPL * dl;
        if (SYS) {
            // (compiler-visible system-scope loads: they stay in flight together with the cache rows requested above)
#pragma unroll
            for (int e = 0; e < EPL / 4; ++e) {
                const hf32x4 rq = ld16_sys_v(base + 4 * e), rk = ld16_sys_v(base + C + 4 * e), rv = ld16_sys_v(base + 2 * C + 4 * e);
#pragma unroll
                for (int i = 0; i < 4; ++i) { q[n][4 * e + i] = rq[i] * 0.125f; k[n][4 * e + i] = rk[i]; v[n][4 * e + i] = rv[i]; }
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) { q[n][e] = base[e] * 0.125f; k[n][e] = base[C + e]; v[n][e] = base[2 * C + e]; }
        }
    }
    // the new position's key / value join the caches (rows `step`: never among the rows read above)
    if (grp == 0) {
#pragma unroll
        for (int n = 0; n < NH; ++n) { kc[n][(size_t)step * rstride] = Wd::pack(k[n]); vc[n][(size_t)step * rstride] = Wd::pack(v[n]); }
    }
    float inv[NH];
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        float cur = 0.0f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) cur = fmaf(q[n][e], k[n][e], cur);
        cur = group_sum<GS>(cur);
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = TPI * i + grp;
            float s = -INFINITY;
            if (TPI * i <= step) {                             // uniform
                float dot = 0.0f;
                if (TPI * i < step) {
                    float kf[EPL];
                    Wd::unpack(kr[n][i], kf);
#pragma unroll
                    for (int e = 0; e < EPL; ++e) dot = fmaf(q[n][e], kf[e], dot);
                    dot = group_sum<GS>(dot);
                }
                if (p == step) dot = cur;
                const bool valid = p <= step && tk[i] != pad_idx;
                s = valid ? dot : -INFINITY;
            }
            sc[n][i] = s;
            mx = fmaxf(mx, s);
        }
        mx = across_groups_max<GS>(mx);
        float l = 0.0f;
#pragma unroll
        for (int i = 0; i < NP; ++i) { sc[n][i] = sc[n][i] == -INFINITY ? 0.0f : expf(sc[n][i] - mx); l += sc[n][i]; }
        l = across_groups_sum<GS>(l);
        inv[n] = 1.0f / l;
    }
    if (!kValuesEarly) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = TPI * i + grp;
            if (TPI * i < step) {
#pragma unroll
                for (int n = 0; n < NH; ++n) vr[n][i] = vc[n][(size_t)(p < step ? p : 0) * rstride];
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NH; ++n) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = TPI * i + grp;
            if (TPI * i <= step) {
                const float pw = sc[n][i] * inv[n];
                if (p == step) {
#pragma unroll
                    for (int e = 0; e < EPL; ++e) acc[e] = fmaf(pw, v[n][e], acc[e]);
                } else if (p < step) {
                    float vf[EPL];
                    Wd::unpack(vr[n][i], vf);
#pragma unroll
                    for (int e = 0; e < EPL; ++e) acc[e] = fmaf(pw, vf[e], acc[e]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = across_groups_sum<GS>(acc[e]);
        if (grp == 0) {
            if (out_cm) {                                      // channel-major (C, Nb): the exact-fp32 step GEMMs' operand layout
#pragma unroll
                for (int e = 0; e < EPL; ++e) out[(size_t)(kDK * (h + n) + EPL * dl + e) * Nb + b] = acc[e];
            } else {
                float* o = out + (size_t)b * C + kDK * (h + n) + EPL * dl;
#pragma unroll
                for (int e = 0; e < EPL; e += 4) {
                    if (SYS) st16_x(o + e, hf32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]}, plain_st);
                    else *reinterpret_cast<float4*>(o + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
                }
            }
        }
    }
    return true;
}

template <typename KV>
__global__ void __launch_bounds__(256)
attn_dec_self_wide_kernel(const float* __restrict__ qkv_t, int C, int Nb, int H, int step, int Lmax,
                          KV* __restrict__ Kc, KV* __restrict__ Vc, const int* __restrict__ tokens, int Lt,
                          int pad_idx, float* __restrict__ out, int out_cm)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int pair = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= Nb * H) return;
    const int b = pair / H, h = pair - b * H;
    self_attend<KV, false>(qkv_t, C, Nb, H, step, Lmax, Kc, Vc, tokens, Lt, pad_idx, out, out_cm, b, h, lane);
}

// ---- decoder, one step: classifier epilogue ------------------------------------------------------------------
// logits (Cc, Nb) channel-major.  Greedy: out[b][step][:] = softmax(logits[:, b]) and
// tokens[b][step+1] = arg-max (first maximum)  (nrtr_decoder.py:168-175).  Forced: out = raw logits.
__global__ void __launch_bounds__(256)
dec_classify_kernel(const float* __restrict__ logits, int Cc, int Nb, int step, int L, int greedy,
                    float* __restrict__ out, int* __restrict__ tokens, int Lt, int tm,
                    const float* __restrict__ emb = nullptr, const float* __restrict__ pos = nullptr,
                    float* __restrict__ x_next = nullptr, int C = 0)
{
    // one wavefront per image, lanes over classes
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= Nb) return;
    float* o = out + ((size_t)b * L + step) * Cc;
    const size_t ls = tm ? 1 : (size_t)Nb;                 // stride between the classes of an image
    logits += tm ? (size_t)b * Cc : (size_t)b;
    // x_next (token-major step pipeline): the next step's embedding row of this image is written here as well, from the
    // token this step decided (or was given) -- one launch per step instead of two
    auto embed_next = [&](int tok) {
        if (x_next) {
            const float* er = emb + (size_t)tok * C;
            const float* pr = pos + (size_t)(step + 1) * C;
            for (int c = lane; c < C; c += kWave) x_next[(size_t)b * C + c] = er[c] + pr[c];
        }
    };
    if (!greedy) {
        for (int c = lane; c < Cc; c += kWave) o[c] = logits[(size_t)c * ls];
        embed_next(tokens[(size_t)b * Lt + step + 1]);
        return;
    }
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = lane; c < Cc; c += kWave) {
        const float v = logits[(size_t)c * ls];
        if (v > mx) { mx = v; am = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(mx, off, kWave);
        const int oi = __shfl_xor(am, off, kWave);
        if (ov > mx || (ov == mx && oi < am)) { mx = ov; am = oi; }
    }
    float sum = 0.0f;
    for (int c = lane; c < Cc; c += kWave) sum += expf(logits[(size_t)c * ls] - mx);
    sum = wave_sum(sum);
    for (int c = lane; c < Cc; c += kWave) o[c] = expf(logits[(size_t)c * ls] - mx) / sum;
    if (lane == 0) tokens[(size_t)b * Lt + step + 1] = am;
    embed_next(am);
}

__global__ void __launch_bounds__(256)
dec_init_tokens_kernel(int* __restrict__ tokens, int Nb, int Lt, int start_idx, int pad_idx,
                       const int* __restrict__ forced, int Lf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nb * Lt) return;
    const int b = i / Lt, p = i - b * Lt;
    if (forced) tokens[i] = p < Lf ? forced[(size_t)b * Lf + p] : pad_idx;
    else tokens[i] = p == 0 ? start_idx : pad_idx;
}

// ---- decoder, one step: the projections on the bf16 matrix cores with the three-term split ------------------------
// out (M, Co) = act(LN?(X) W + bias) [+ res], all TOKEN-major, X (M, K) fp32, M = images of the step.
// Why not the fp32 split-K kernel (conv1x1_skinny_f32_kernel) the exact-fp32 configuration keeps: its operands arrive
// as 4-byte loads (512 load instructions per 32x32 tile at 16 cycles each in the vector-memory unit: 3.7 us of an 8 us
// launch) and meet in 16 partial tiles of 64 KB.  Here
//   * the MFMA runs  D[co][token] = W^T[co][k] X^T[k][token]  so that a lane's B fragment is 8 consecutive k of ITS
//     token -- two 16-byte loads of the token-major row -- and its results are 4 consecutive outputs of its token
//     (16-byte stores);
//   * the weight arrives pre-split (hi = bf16(w), lo = bf16(w - hi)) and pre-arranged on the host in fragment order,
//     [Co/32][K/16][hi|lo][k half][32 outputs][8 k]: a fragment is one 16-byte load, a wavefront load 1 KB contiguous;
//   * x is split in registers (two v_cvt_pk_bf16_f32 and a subtraction per pair); a product is hi*hi + hi*lo + lo*hi
//     accumulated in fp32 (~5e-6 of a layer's scale, as in tpspp_conv2d_bf16_fwd's split3);
//   * four wavefronts split K (K/64 MFMA k-steps each, every load of a wavefront in flight together), four partial
//     tiles meet in 16 KB of LDS;
//   * LayerNorm folded by the identity of tpspp_linear_ln_fwd, but on the RAW row: its sum and sum of squares ride on the
//     same loads.  (tpspp_linear_ln_fwd shifts every column by the median of three of its values first; this kernel does
//     not, so the two differ numerically once |mean| >> std of a token: include/tpspp.h gives that kernel's figures.)
struct DGemm {
    const float* X; const u32x4* Wp; const float* bias; const float* colsum; const float* res; float* out;
    int M, K, Co;            // Co: valid outputs (the arranged weight is padded to a multiple of 32)
    float eps; int act;      // act: 0 none, 2 GELU (erf)
    int remap = 0;           // dec_gemm_tile
};

// Workgroup -> (token block, output tile) for the step GEMMs.  Workgroups go to the 8 XCDs round-robin in launch order and
// every XCD has its own L2, which each launch fills with the X rows (the previous launch's output) and the W tiles its
// workgroups touch.  In launch order an XCD gets 2 of the 16 token blocks and ALL output tiles; scripts/ubench/gemm_chain_bench
// (the projection's loads alone, 2000 dependent launches): launch order 5.03 us, 4 token blocks x half the tiles 4.77 us,
// 8 x a quarter 5.30 us, all 16 x an eighth 5.56 us -- X, freshly written elsewhere, costs more per byte than W.
// In the decoder (same box, interleaved): bf16 15.36 -> 15.19 ms, bf16x3 20.49 -> 20.42 ms, exact fp32 23.24 -> 23.30 (left
// in launch order).  Only the 16-token-block grids of batch 512 with an even number of tile rows are remapped.
__device__ __forceinline__ void dec_gemm_tile(int& bx, int& by, bool remap)
{
    bx = blockIdx.x; by = blockIdx.y;
    if (remap && gridDim.x == 16 && (gridDim.y & 1) == 0) {
        const int lin = blockIdx.x + 16 * blockIdx.y, xcd = lin & 7, slot = lin >> 3;
        bx = (xcd & 3) * 4 + (slot & 3);
        by = (xcd >> 2) * (gridDim.y >> 1) + (slot >> 2);
    }
}

// NT: 32-output tiles per workgroup (1; 3 for the 1536-wide q|k|v projection: at one tile per workgroup its 768 workgroups
// ran as two rounds of latency-bound launches -- ~14 us against 6.5 us for the 512-wide projections -- while three tiles per
// workgroup are one round of 256 and read X once instead of three times; every tile is computed exactly as before).
template <int KSW, bool LN, int NT = 1>
__global__ void __launch_bounds__(256)
dec_gemm_x3_kernel(const DGemm P)
{
    __shared__ float sRed[4][16][kWave];
    __shared__ float sS1[8][32], sS2[8][32];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    int bx, by;
    dec_gemm_tile(bx, by, P.remap != 0);
    const int m0 = bx * 32, ct0 = by * NT;
    const int KS = P.K >> 4;
    const int m = m0 + l31;
    const int mc = m < P.M ? m : P.M - 1;
    const int ntiles = (P.Co + 31) >> 5;
    const float4* xp = reinterpret_cast<const float4*>(P.X + (size_t)mc * P.K + 16 * (wv * KSW) + 8 * half);
    float4 xa[KSW][2];
    u32x4 ah[NT][KSW], al[NT][KSW];
#pragma unroll
    for (int j = 0; j < KSW; ++j) { xa[j][0] = xp[4 * j]; xa[j][1] = xp[4 * j + 1]; }   // every load of the wavefront in flight together
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const int ct = ct0 + tl < ntiles ? ct0 + tl : ntiles - 1;     // (a tile past the last one repeats it; never finished)
        const u32x4* wp = P.Wp + ((size_t)(ct * KS + wv * KSW) * 4 + half) * 32 + l31;
#pragma unroll
        for (int j = 0; j < KSW; ++j) { ah[tl][j] = wp[(size_t)j * 128]; al[tl][j] = wp[(size_t)j * 128 + 64]; }
    }
    // ... and the epilogue's operands with them (round 4): behind the reduction they were one more dependent round trip
    // to memory per launch, in a loop of ~2000 dependent launches
    bool mine[NT];
    size_t o[NT];
    float4 cs[NT], b4[NT], r4[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const int c = (ct0 + tl) * 32 + 8 * wv + 4 * half;
        mine[tl] = m < P.M && c < P.Co;                    // (Co is a multiple of 4: a whole piece is in or out)
        o[tl] = (size_t)mc * P.Co + (c < P.Co ? c : 0);
        cs[tl] = make_float4(0.f, 0.f, 0.f, 0.f); b4[tl] = cs[tl]; r4[tl] = cs[tl];
        if (mine[tl]) {
            if (LN) cs[tl] = *reinterpret_cast<const float4*>(P.colsum + c);
            if (P.bias) b4[tl] = *reinterpret_cast<const float4*>(P.bias + c);
            if (P.res) r4[tl] = *reinterpret_cast<const float4*>(P.res + o[tl]);
        }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tl][i] = 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < KSW; ++j) {
        const float x[8] = {xa[j][0].x, xa[j][0].y, xa[j][0].z, xa[j][0].w, xa[j][1].x, xa[j][1].y, xa[j][1].z, xa[j][1].w};
        u32x4 bh, bl;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned pk = pack_bf16(x[2 * q], x[2 * q + 1]);
            const float h0 = __builtin_bit_cast(float, pk << 16), h1 = __builtin_bit_cast(float, pk & 0xffff0000u);
            bh[q] = pk;
            bl[q] = pack_bf16(x[2 * q] - h0, x[2 * q + 1] - h1);
            if (LN) {
                s1 += x[2 * q] + x[2 * q + 1];
                s2 = fmaf(x[2 * q], x[2 * q], s2);
                s2 = fmaf(x[2 * q + 1], x[2 * q + 1], s2);
            }
        }
        const bf16x8 Bh = __builtin_bit_cast(bf16x8, bh), Bl = __builtin_bit_cast(bf16x8, bl);
#pragma unroll
        for (int tl = 0; tl < NT; ++tl) {
            const bf16x8 Ah = __builtin_bit_cast(bf16x8, ah[tl][j]), Al = __builtin_bit_cast(bf16x8, al[tl][j]);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bh, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Ah, Bl, acc[tl], 0, 0, 0);
            acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Al, Bh, acc[tl], 0, 0, 0);
        }
    }
    if (LN) { sS1[wv * 2 + half][l31] = s1; sS2[wv * 2 + half][l31] = s2; }
    float mean = 0.0f, rstd = 1.0f;
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        if (tl > 0) __syncthreads();                       // the previous tile's partial sums have been read
#pragma unroll
        for (int r = 0; r < 16; ++r) sRed[wv][r][lane] = acc[tl][r];
        __syncthreads();
        // wavefront w finishes accumulator registers 4 w .. 4 w + 3: outputs 32 ct + 8 w + 4 half + (0 .. 3) of token l31
        if (LN && tl == 0) {
            float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { t1 += sS1[j][l31]; t2 += sS2[j][l31]; }
            mean = t1 / (float)P.K;
            rstd = 1.0f / sqrtf(fmaxf(t2 / (float)P.K - mean * mean, 0.0f) + P.eps);
        }
        if (!mine[tl]) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            v[e] = (sRed[0][4 * wv + e][lane] + sRed[1][4 * wv + e][lane]) + (sRed[2][4 * wv + e][lane] + sRed[3][4 * wv + e][lane]);
        if (LN) {
            v[0] = rstd * (v[0] - mean * cs[tl].x); v[1] = rstd * (v[1] - mean * cs[tl].y);
            v[2] = rstd * (v[2] - mean * cs[tl].z); v[3] = rstd * (v[3] - mean * cs[tl].w);
        }
        if (P.bias) { v[0] += b4[tl].x; v[1] += b4[tl].y; v[2] += b4[tl].z; v[3] += b4[tl].w; }
        if (P.act == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
        }
        if (P.res) { v[0] += r4[tl].x; v[1] += r4[tl].y; v[2] += r4[tl].z; v[3] += r4[tl].w; }
        *reinterpret_cast<float4*>(P.out + o[tl]) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

#include "tpspp_head_persist.h"

// The same GEMM with exact fp32 products (v_mfma_f32_32x32x2_f32) for the exact-fp32 configuration: the weight arrives
// as fp32 in fragment order, [Co/32][K/8][k half][32 outputs][4 k] with k = 8 u + 4 half + e, x as 16-byte pieces of the
// token-major row (the lane's four k of the step), four MFMAs per 16-byte pair; eight wavefronts split K.
struct DGemmF {
    const float* X; const float4* Wp; const float* bias; const float* colsum; const float* res; float* out;
    int M, K, Co; float eps; int act;
    int remap = 0;
};
template <int KUW, bool LN, int NT = 1>
__global__ void __launch_bounds__(512)
dec_gemm_f32_kernel(const DGemmF P)
{
    __shared__ float sRed[8][16][kWave];
    __shared__ float sS1[16][32], sS2[16][32];
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    int bx, by;
    dec_gemm_tile(bx, by, P.remap != 0);
    const int m0 = bx * 32, ct0 = by * NT;
    const int KU = P.K >> 3;
    const int m = m0 + l31;
    const int mc = m < P.M ? m : P.M - 1;
    const int ntiles = (P.Co + 31) >> 5;
    const float4* xp = reinterpret_cast<const float4*>(P.X + (size_t)mc * P.K + 8 * (wv * KUW) + 4 * half);
    float4 xa[KUW], wa[NT][KUW];
#pragma unroll
    for (int j = 0; j < KUW; ++j) xa[j] = xp[2 * j];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const int ct = ct0 + tl < ntiles ? ct0 + tl : ntiles - 1;
        const float4* wp = P.Wp + ((size_t)(ct * KU + wv * KUW) * 2 + half) * 32 + l31;
#pragma unroll
        for (int j = 0; j < KUW; ++j) wa[tl][j] = wp[(size_t)j * 64];
    }
    // the epilogue's operands ride with them (wavefronts 0 - 3 finish the tile; see dec_gemm_x3_kernel)
    bool mine[NT];
    size_t o[NT];
    float4 cs[NT], b4[NT], r4[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        const int c = (ct0 + tl) * 32 + 8 * (wv & 3) + 4 * half;
        mine[tl] = wv < 4 && m < P.M && c < P.Co;
        o[tl] = (size_t)mc * P.Co + (c < P.Co ? c : 0);
        cs[tl] = make_float4(0.f, 0.f, 0.f, 0.f); b4[tl] = cs[tl]; r4[tl] = cs[tl];
        if (mine[tl]) {
            if (LN) cs[tl] = *reinterpret_cast<const float4*>(P.colsum + c);
            if (P.bias) b4[tl] = *reinterpret_cast<const float4*>(P.bias + c);
            if (P.res) r4[tl] = *reinterpret_cast<const float4*>(P.res + o[tl]);
        }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int tl = 0; tl < NT; ++tl)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[tl][i] = 0.0f;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < KUW; ++j) {
        const float x[4] = {xa[j].x, xa[j].y, xa[j].z, xa[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (LN) { s1 += x[e]; s2 = fmaf(x[e], x[e], s2); }
#pragma unroll
            for (int tl = 0; tl < NT; ++tl) {
                const float w = e == 0 ? wa[tl][j].x : e == 1 ? wa[tl][j].y : e == 2 ? wa[tl][j].z : wa[tl][j].w;
                acc[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, x[e], acc[tl], 0, 0, 0);
            }
        }
    }
    if (LN) { sS1[wv * 2 + half][l31] = s1; sS2[wv * 2 + half][l31] = s2; }
    float mean = 0.0f, rstd = 1.0f;
#pragma unroll
    for (int tl = 0; tl < NT; ++tl) {
        if (tl > 0) __syncthreads();                       // the previous tile's partial sums have been read
#pragma unroll
        for (int r = 0; r < 16; ++r) sRed[wv][r][lane] = acc[tl][r];
        __syncthreads();
        // wavefronts 0 - 3 finish accumulator registers 4 w .. 4 w + 3: outputs 32 ct + 8 w + 4 half + (0 .. 3) of token l31
        if (LN && tl == 0) {
            float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) { t1 += sS1[j][l31]; t2 += sS2[j][l31]; }
            mean = t1 / (float)P.K;
            rstd = 1.0f / sqrtf(fmaxf(t2 / (float)P.K - mean * mean, 0.0f) + P.eps);
        }
        if (!mine[tl]) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = 0.0f;
#pragma unroll
            for (int pz = 0; pz < 8; pz += 2) t += sRed[pz][4 * wv + e][lane] + sRed[pz + 1][4 * wv + e][lane];
            v[e] = t;
        }
        if (LN) {
            v[0] = rstd * (v[0] - mean * cs[tl].x); v[1] = rstd * (v[1] - mean * cs[tl].y);
            v[2] = rstd * (v[2] - mean * cs[tl].z); v[3] = rstd * (v[3] - mean * cs[tl].w);
        }
        if (P.bias) { v[0] += b4[tl].x; v[1] += b4[tl].y; v[2] += b4[tl].z; v[3] += b4[tl].w; }
        if (P.act == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
        }
        if (P.res) { v[0] += r4[tl].x; v[1] += r4[tl].y; v[2] += r4[tl].z; v[3] += r4[tl].w; }
        *reinterpret_cast<float4*>(P.out + o[tl]) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ===== AttnConvertor.tensor2idx on the device (round 6) =================================================================
// scores (N, L, C): per position the maximum and its FIRST index (torch.max's tie rule; a NaN beats every number, as in ATen's
// reduction), then the reference's scan per image -- skip <PAD>, stop at the first <EOS> (convertors/attn.py:124-137) -- so that
// the host needs ONE copy of (N, L) indices + (N, L) scores instead of the score tensor's arg-max in fp64 and a Python scan.
// One wavefront per image: lanes over classes while reducing a position, lane = position while scanning.
__global__ void __launch_bounds__(256)
attn_tensor2idx_kernel(const float* __restrict__ scores, int N, int L, int C, int end_idx, int pad_idx,
                       int* __restrict__ idx_out, float* __restrict__ val_out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= N) return;
    bool ended = false;                                     // (wave-uniform)
    for (int l0 = 0; l0 < L; l0 += kWave) {
        const int nl = L - l0 < kWave ? L - l0 : kWave;
        float my_v = 0.0f;
        int my_i = -1;
        for (int j = 0; j < nl; ++j) {
            const float* row = scores + ((size_t)b * L + l0 + j) * C;
            float mx = -INFINITY;
            int am = 0x7fffffff;
            bool nan = false;
            for (int c = lane; c < C; c += kWave) {
                const float v = row[c];
                if (!nan && (v != v)) { nan = true; mx = v; am = c; }
                else if (!nan && (v > mx || am == 0x7fffffff)) { mx = v; am = c; }   // (first element always taken: a row of -inf has index 0)
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(mx, off, kWave);
                const int oi = __shfl_xor(am, off, kWave);
                const bool on = __shfl_xor((int)nan, off, kWave) != 0;
                const bool take = oi != 0x7fffffff &&
                                  (am == 0x7fffffff || (on && !nan) || (on == nan && (on ? oi < am : (ov > mx || (ov == mx && oi < am)))));
                if (take) { mx = ov; am = oi; nan = on; }
            }
            if (lane == j) { my_v = mx; my_i = am; }
        }
        const bool valid = lane < nl;
        const unsigned long long ends = __ballot(valid && my_i == end_idx);
        const int first_end = ended ? 0 : (ends ? __ffsll((long long)ends) - 1 : kWave);
        if (valid) {
            const bool keep = lane < first_end && my_i != pad_idx;
            idx_out[(size_t)b * L + l0 + lane] = keep ? my_i : -1;
            val_out[(size_t)b * L + l0 + lane] = my_v;
        }
        ended = ended || ends != 0;
    }
}
