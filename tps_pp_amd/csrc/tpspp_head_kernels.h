// Device code of the recogniser head, first part: re-layouts, LayerNorm and the encoder self-attention (and the laboratory
// kernel of tpspp_lab_occupy).  Included by tpspp_head.hip inside its anonymous namespace; tpspp_head_step.h follows it.
#pragma once

constexpr int kDK = 64;                 // head width (d_k = d_v = 64: every NRTR config of the reference)
constexpr int kKRow = kDK + 4;          // LDS row stride of the staged keys / values (16-B aligned rows)

// ---- re-layouts ---------------------------------------------------------------------------------
// (N, C, T) -> (C, N*T): out[c][b*T + t] = in[b][c][t]   (rows of T stay contiguous on both sides)
__global__ void __launch_bounds__(256)
nct_to_cm_kernel(const float* __restrict__ in, int N, int C, int T, float* __restrict__ out)
{
    const size_t total = (size_t)N * C * T;
    const size_t M = (size_t)N * T;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / M, m = i - c * M;
        const size_t b = m / T, t = m - b * T;
        out[i] = in[(b * C + c) * T + t];
    }
}

// out (cols, rows) = in (rows, cols)^T through a padded 32x32 LDS tile
__global__ void __launch_bounds__(256)
transpose2d_kernel(const float* __restrict__ in, int rows, int cols, float* __restrict__ out)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int r = r0 + ty + k, c = c0 + tx;
        tile[ty + k][tx] = (r < rows && c < cols) ? in[(size_t)r * cols + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int c = c0 + ty + k, r = r0 + tx;
        if (c < cols && r < rows) out[(size_t)c * rows + r] = tile[tx][ty + k];
    }
}

// ---- LayerNorm over the rows of a channel-major matrix ----------------------------------------------
// y[c][m] = (x[c][m] - mean_m) * rstd_m * gamma[c] + beta[c];  mean / biased variance over c.
// Workgroup = 16 columns x 16 interleaved channel slices; a thread keeps its C/16 values in registers
// (one pass over x, all loads in flight together: a decoder step has only a few hundred columns, so
// the kernel is latency-bound unless every load is issued up front).  C <= 16 * VPT.
// (round 6: compiled for three workgroups per CU -- VPT = 32 took 176 registers, two wavefronts per SIMD, in a kernel that only
// waits for memory)
template <int VPT>
__global__ void __launch_bounds__(256, VPT <= 32 ? 3 : 1)
layernorm_cm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                    int C, int M, float eps, float* __restrict__ y)
{
    __shared__ float red[16][17];
    const int col = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int m = blockIdx.x * 16 + col;
    const bool ok = m < M;
    const int mm = ok ? m : M - 1;
    float v[VPT], g[VPT], be[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {                    // every load of the thread issued up front
        const int c = sl + 16 * i;
        const int cc = c < C ? c : C - 1;
        v[i] = x[(size_t)cc * M + mm];
        g[i] = gamma[cc];
        be[i] = beta[cc];
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) s += (sl + 16 * i) < C ? v[i] : 0.0f;
    red[sl][col] = s;
    __syncthreads();
    float tot = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += red[j][col];
    const float mean = tot / (float)C;
    __syncthreads();
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const float d = (sl + 16 * i) < C ? v[i] - mean : 0.0f;
        q = fmaf(d, d, q);
    }
    red[sl][col] = q;
    __syncthreads();
    tot = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; ++j) tot += red[j][col];
    const float rstd = 1.0f / sqrtf(tot / (float)C + eps);
    if (!ok) return;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int c = sl + 16 * i;
        if (c < C) y[(size_t)c * M + m] = (v[i] - mean) * rstd * g[i] + be[i];
    }
}

// ---- encoder self-attention -------------------------------------------------------------------------
// qkv (3C, M) channel-major, M = N*T; head h of image b: rows [64h, 64h+64) of each third, columns
// [bT, bT+T).  Workgroup = one (image, head, block of <=256 queries): the head's keys and values are
// staged in LDS ([key][feature], read back as wavefront-wide broadcasts), one query per thread with q
// and the output accumulator in registers.  Two passes over the keys (row maximum, then exp / sum /
// weighted values): scores are recomputed rather than stored, so T is bounded only by LDS (T <= 256).
// Keys >= valid_len[b] are masked (nrtr_encoder.py:51-65: the first ceil(T*valid_ratio) tokens count).
__global__ void __launch_bounds__(256)
attn_enc_kernel(const float* __restrict__ qkv, int C, int M, int T, const int* __restrict__ valid_len,
                float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;                         // [T][kKRow]
    float* Vs = smem + (size_t)T * kKRow;
    const int b = blockIdx.z, h = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const size_t col0 = (size_t)b * T;
    // staging: 8 key rows + 8 value rows per wavefront in flight (a one-wavefront workgroup would
    // otherwise pay a full memory latency for each of its 128 rows)
    for (int j0 = 0; j0 < T; j0 += kWave) {
        const int j = j0 + lane;
        const int jj = j < T ? j : T - 1;
        for (int d0 = wv; d0 < kDK; d0 += 8 * nw) {
            float kk[8], vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int d = d0 + u * nw < kDK ? d0 + u * nw : wv;
                kk[u] = qkv[(size_t)(C + kDK * h + d) * M + col0 + jj];
                vv[u] = qkv[(size_t)(2 * C + kDK * h + d) * M + col0 + jj];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int d = d0 + u * nw;
                if (d < kDK && j < T) {
                    Ks[j * kKRow + d] = kk[u];
                    Vs[j * kKRow + d] = vv[u];
                }
            }
        }
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    int nvalid = valid_len ? valid_len[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    float q[kDK];
#pragma unroll
    for (int d = 0; d < kDK; ++d) q[d] = qkv[(size_t)(kDK * h + d) * M + col0 + i] * 0.125f;   // q / sqrt(d_k)

    auto score = [&](int j) {
        const float4* kr = reinterpret_cast<const float4*>(Ks + j * kKRow);
        float s = 0.0f;
#pragma unroll
        for (int d4 = 0; d4 < kDK / 4; ++d4) {
            const float4 kv = kr[d4];
            s = fmaf(q[4 * d4 + 0], kv.x, s);
            s = fmaf(q[4 * d4 + 1], kv.y, s);
            s = fmaf(q[4 * d4 + 2], kv.z, s);
            s = fmaf(q[4 * d4 + 3], kv.w, s);
        }
        return s;
    };
    float mx = -INFINITY;
    for (int j = 0; j < nvalid; ++j) mx = fmaxf(mx, score(j));
    float acc[kDK];
#pragma unroll
    for (int d = 0; d < kDK; ++d) acc[d] = 0.0f;
    float l = 0.0f;
    for (int j = 0; j < nvalid; ++j) {
        const float p = expf(score(j) - mx);
        l += p;
        const float4* vr = reinterpret_cast<const float4*>(Vs + j * kKRow);
#pragma unroll
        for (int d4 = 0; d4 < kDK / 4; ++d4) {
            const float4 vv = vr[d4];
            acc[4 * d4 + 0] = fmaf(p, vv.x, acc[4 * d4 + 0]);
            acc[4 * d4 + 1] = fmaf(p, vv.y, acc[4 * d4 + 1]);
            acc[4 * d4 + 2] = fmaf(p, vv.z, acc[4 * d4 + 2]);
            acc[4 * d4 + 3] = fmaf(p, vv.w, acc[4 * d4 + 3]);
        }
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int d = 0; d < kDK; ++d) out[(size_t)(kDK * h + d) * M + col0 + i] = acc[d] * inv;
}

// ---- encoder self-attention on the fp32 matrix cores (T <= 128) ----------------------------------------------------
// One wavefront = 32 queries of one (image, head).  Both products are v_mfma_f32_32x32x2_f32 with operands
// taken straight from the channel-major rows (a fragment = two 128-B row segments), nothing staged:
//   S^T tile (32 keys x 32 queries) = sum_d K[d][j] Q[d][i]   -> in the C/D layout a LANE is a QUERY and its
//     16 registers are 16 keys (the other 16 keys of the tile sit in lane^32), so the softmax is a
//     per-lane reduction plus one exchange with lane^32;
//   O^T tile (32 features x 32 queries) = sum_j V[d][j] P^T[j][i]: the probabilities are consumed as the B
//     operand IN PLACE -- register r of lane (i, half) holds key 8*(r>>2) + (r&3) + 4*half of its tile, and
//     those two keys (half = 0, 1) are taken as the k-pair of MFMA step r; the A operand reads V at the
//     same two keys.  No LDS, no barrier.
// NJ = ceil(T / 32) key tiles (template, <= 4).  Scores are scaled by 1/8 through q, keys >= valid_len[b]
// get probability 0 and their V columns are not read (the index is clamped to the last valid key), so whatever a
// masked column of k or v holds, NaN included, cannot reach the output.
// (round 6: compiled for three workgroups per CU -- NJ = 2, the 64-token case, took 172 registers = two wavefronts per SIMD,
// 168 is three; the kernel waits for memory)
template <int NJ>
__global__ void __launch_bounds__(256, NJ <= 2 ? 3 : 1)
attn_enc_mfma_kernel(const float* __restrict__ qkv, int C, int M, int T, const int* __restrict__ valid_len,
                     float* __restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int half = lane >> 5, l31 = lane & 31;
    const int nib = (T + 31) >> 5;                           // query blocks per (image, head)
    const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int H = C / kDK;
    const int ib = w % nib, bh = w / nib;
    if (bh >= (M / T) * H) return;                           // wave-uniform (M / T = images)
    const int h = bh % H, b = bh / H;
    const size_t col0 = (size_t)b * T;
    int nvalid = valid_len ? valid_len[b] : T;
    nvalid = nvalid < T ? nvalid : T;
    const int jlast = nvalid > 0 ? nvalid - 1 : 0;           // the last valid key: what a masked V column index is clamped to
    const int i = ib * 32 + l31;                             // this lane's query (B-operand column)
    const int ic = i < T ? i : T - 1;
    const float* qp = qkv + (size_t)(kDK * h) * M + col0;
    const float* kp = qkv + (size_t)(C + kDK * h) * M + col0;
    const float* vp = qkv + (size_t)(2 * C + kDK * h) * M + col0;

    // B fragments of Q for all 32 k-steps (k = feature pair 2*ks + half), scaled
    float qf[32];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) qf[ks] = qp[(size_t)(2 * ks + half) * M + ic] * 0.125f;

    f32x16 sc[NJ];
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[jb][r] = 0.0f;
        const int j = jb * 32 + l31;                         // A-operand row: key
        const int jc = j < T ? j : T - 1;
        float kf[32];
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) kf[ks] = kp[(size_t)(2 * ks + half) * M + jc];
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) sc[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[ks], qf[ks], sc[jb], 0, 0, 0);
    }
    // softmax over the keys of query i: registers of this lane + the complementary keys in lane^32
    float mx = -INFINITY;
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            sc[jb][r] = j < nvalid ? sc[jb][r] : -INFINITY;
            mx = fmaxf(mx, sc[jb][r]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
    float l = 0.0f;
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = sc[jb][r] == -INFINITY ? 0.0f : expf(sc[jb][r] - mx);
            sc[jb][r] = p;
            l += p;
        }
    l += __shfl_xor(l, 32, kWave);
    const float inv = 1.0f / l;

    // O^T = V P^T, two feature tiles of 32
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.0f;
        const float* vrow = vp + (size_t)(dt * 32 + l31) * M;   // A-operand row: feature
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) {
            float vf[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                vf[r] = vrow[j < nvalid ? j : jlast];             // a masked column is never read: 0 x NaN would reach o
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[r], sc[jb][r], o, 0, 0, 0);
        }
        if (i < T) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                out[(size_t)(kDK * h + d) * M + col0 + i] = o[r] * inv;
            }
        }
    }
}

// (rows, cols) bf16 -> (cols, rows) bf16, 64x64 tiles through LDS
__global__ void __launch_bounds__(256)
transpose2d_b16_kernel(const unsigned short* __restrict__ in, int rows, int cols, unsigned short* __restrict__ out)
{
    __shared__ unsigned short tile[64][66];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? in[(size_t)r * cols + c] : (unsigned short)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) out[(size_t)c * rows + r] = tile[tx][i];
    }
}

// lab / test kernel (tpspp_lab_occupy): `blocks` workgroups that hold `lds` bytes of LDS each and spin on the wall clock
__global__ void __launch_bounds__(64) lab_occupy_kernel(long long ticks, int* sink)
{
    extern __shared__ int occ_smem[];
    const long long t0 = (long long)wall_clock64();
    int n = 0;
    while ((long long)wall_clock64() - t0 < ticks) { __builtin_amdgcn_s_sleep(64); ++n; }
    if (n < 0) { occ_smem[threadIdx.x] = n; sink[0] = occ_smem[0]; }       // (never: keeps the LDS allocation alive)
}
