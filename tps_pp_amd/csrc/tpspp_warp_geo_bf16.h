// Classic-geometry warp with bf16 images in and out (TPSPP_IO_BF16 with the prepared table): the run-time-geometry in-place
// kernel of tpspp_warp_geo.h, one image per workgroup, with both ends narrowed to bf16.  Parameter record (GeoParams), LDS
// byte count (geo_lds_bytes with 2-byte planes), planner and launchers are that kernel's (tpspp_warp_geo.hip).
//
// The arithmetic is that of the fp32 in-place kernels, unchanged: T rows and grid coordinates are the k-ascending fp32 FMA
// chains from zero, the tap descriptors are make_taps_lite()'s, the four-tap blend is the same three fp32 FMAs behind one
// product.  Compiled with -ffp-contract=off.  Only the two ends differ:
//   * the image is bf16 in HBM and in LDS (half the DMA pieces, half the LDS).  Its planes keep the layout they have in
//     HBM, two pixels per 32-bit LDS word.  A tap is ONE 16-bit LDS read (ds_read_u16: the word's bank, the low or high
//     half by address bit 1), widened exactly by << 16.  The west / east pair of a tap sits in one word when x0 is even and
//     straddles two words when x0 is odd; two 16-bit reads serve both cases with the same instructions, no select and no
//     read that is not naturally aligned -- the LDS instruction count is that of the fp32 kernel (four per pixel and channel).
//   * the fp32 result is rounded to nearest even ONCE (v_cvt_pk_bf16_f32 on the (west, east) mirror pixels of a channel),
//     staged as 16-bit LDS writes in place of the image in the output's own layout -- which packs two pixels per 32-bit
//     word --, and leaves as flat 16-byte nt stores of eight pixels.
// grid_or_null / idx_or_null are fp32 / int32 with the bits the fp32 kernels write.
// A thread holds its results packed (two per register), so the register budget of tpspp_warp_geo.h (QP x C <= 12 results
// per mirror pixel at 12 wavefronts) is met with room: no instantiation has a private segment (tests/test_no_new_scratch.py).
// Large images: as in tpspp_warp_geo.h, `bands` workgroups share an image, each staging the WHOLE image (at two bytes per
// pixel 64x256x3 is 96 KB) and expanding, sampling and writing only its own row groups and their mirror rows.
#pragma once
#include "tpspp_warp_geo.h"

namespace tpspp_geo {

template <int F, int C, int QP, bool AUX>
__global__ void __launch_bounds__(geo_max_threads<QP>())
tps_warp_geo_bf16_kernel(const GeoParams P)
{
    constexpr int K = F + 3;
    const int H = P.H, W = P.W, HW = H * W, img_elems = C * HW;
    const int BW = P.BW, BH = 32 / BW, CG = P.CG, NW = P.NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* sT = reinterpret_cast<float2*>(smem);           // [K]
    float* sFlag = smem + ((2 * K + 3) & ~3);               // [0] T rows published, [1] loaders done
    char* sImg = reinterpret_cast<char*>(smem + P.img_off);

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int b = blockIdx.x / P.bands, band = blockIdx.x - b * P.bands;
    const int NLOAD = (int)(blockDim.x / kWave) - NW;

    // T-solve inputs first (wavefront 0; lane i keeps control point i and row i of inv_delta_C, 16 bytes at a time: the
    // last piece starts at column K - 4 so that the last row does not read past the matrix)
    constexpr int KGI = (K + 3) / 4;
    float hrowv[KGI * 4];
    float cx = 0.0f, cy = 0.0f;
    if (wv == 0) {
        if (lane < F) {
            const float2 cc = reinterpret_cast<const float2*>(P.ctrl + (size_t)b * F * 2)[lane];
            cx = cc.x; cy = cc.y;
        }
        const float* row = P.inv_delta_c + (lane < K ? lane : K - 1) * K;
#pragma unroll
        for (int j = 0; j < KGI; ++j) {
            const int c0 = (j == KGI - 1) ? K - 4 : 4 * j;
            const v4f_a4 x = *reinterpret_cast<const v4f_a4*>(row + c0);
            hrowv[4 * j] = x[0]; hrowv[4 * j + 1] = x[1]; hrowv[4 * j + 2] = x[2]; hrowv[4 * j + 3] = x[3];
        }
    }
    if (tid < 4) reinterpret_cast<int*>(sFlag)[tid] = 0;
    lds_only_barrier();                                      // the only barrier every wavefront takes part in

    if (wv >= NW) {
        // ================= loader wavefronts: 1 KB (512 pixels) per instruction =================
        const int lw = wv - NW;
        const int total_bytes = img_elems * 2;
        const int pieces = (total_bytes + 1023) >> 10;
        const char* src = reinterpret_cast<const char*>(static_cast<const unsigned short*>(P.in) + (size_t)b * img_elems);
        // the flag operands live in registers BEFORE the first DMA, the update is inline asm (tpspp_warp_pair.h)
        unsigned fa = (unsigned)(size_t)(sFlag + 1);
        int one = 1;
        asm volatile("" : "+v"(fa), "+v"(one));
        for (int piece = lw; piece < pieces; piece += NLOAD) {
            int off = piece * 1024 + lane * 16;
            if (off >= total_bytes) off = 0;                 // tail lanes re-read a valid address (their bytes land in the last piece's pad)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(src + off),
                (__attribute__((address_space(3))) void*)(sImg + piece * 1024),
                16, 0, 2 /* nt */);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) tpspp_pair::flag_add<0>(fa, one);
        return;
    }

    // ================= compute wavefronts =================
    // thread -> its QP quadrant pixels, as in tpspp_warp_geo.h
    const bool live = tid < P.nthr;                          // (the last wavefront may be half empty)
    const int tt = live ? tid : P.nthr - 1;
    const int hw = tt >> 5, l5 = tt & 31;
    const int rgb_l = hw / CG, cg = hw - rgb_l * CG;
    const int rgb = band * (P.RGB / P.bands) + rgb_l;
    const int c = cg * BW + (l5 & (BW - 1));                 // BW is a power of two; c < W (CG BW <= W)
    const int r0 = rgb * QP * BH + l5 / BW;                  // quadrant pixel j sits BH rows further per j
    auto pixel_idx = [&](int j, int m) -> unsigned {         // pixel index inside a plane of mirror pixel m of quadrant pixel j
        const int r = r0 + j * BH;
        const int rr = (m & 2) ? H - 1 - r : r, cc = (m & 1) ? W - 1 - c : c;
        return (unsigned)(rr * W + cc);
    };

    // packed table: [wavefront][QP][KG][lane] x 16 bytes in the thread order of the whole quadrant
    constexpr int KG = (K + 3) / 4;
    float v[QP][KG * 4];
    {
        const int t_glob = (rgb * CG + cg) * 32 + l5;
        const v4f* pk = reinterpret_cast<const v4f*>(P.packed) + (size_t)(t_glob >> 6) * QP * KG * kWave + (t_glob & (kWave - 1));
#pragma unroll
        for (int j = 0; j < QP; ++j)
#pragma unroll
            for (int g = 0; g < KG; ++g) {
                const v4f x = pk[(j * KG + g) * kWave];
                v[j][4 * g] = x[0]; v[j][4 * g + 1] = x[1]; v[j][4 * g + 2] = x[2]; v[j][4 * g + 3] = x[3];
            }
    }
    if (wv == 0) {
        float ax = 0.0f, ay = 0.0f;
        static_for<K>([&](auto qc) {                         // ordered broadcast: the sum is the reference's FMA chain
            constexpr int q = decltype(qc)::value;
            constexpr int idx = (q / 4 < KGI - 1) ? q : 4 * (KGI - 1) + (q - (K - 4));
            ax = fmaf(hrowv[idx], readlane_f(cx, q), ax);
            ay = fmaf(hrowv[idx], readlane_f(cy, q), ay);
        });
        if (lane < K) sT[lane] = make_float2(ax, ay);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(reinterpret_cast<int*>(sFlag), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    wait_flag_lds(sFlag + 0, 1);
    asm volatile("" ::"v"(v[QP - 1][KG * 4 - 1]));           // (keeps the table's padding register from being recycled early)

    // ---- 8 QP FMA chains: QP quadrant pixels x 4 mirror pixels x (x, y), each k-ascending from zero ----
    float gx[QP][4], gy[QP][4];
#pragma unroll
    for (int j = 0; j < QP; ++j)
#pragma unroll
        for (int m = 0; m < 4; ++m) gx[j][m] = gy[j][m] = 0.0f;
    static_for<K>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const float2 t = sT[q];
#pragma unroll
        for (int j = 0; j < QP; ++j) {
            float val[4];
            mirror_vals<F, q>(v[j], val);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                gx[j][m] = fmaf(val[m], t.x, gx[j][m]);
                gy[j][m] = fmaf(val[m], t.y, gy[j][m]);
            }
        }
    });

    typedef __attribute__((address_space(3))) const unsigned short lds_cu16;
    typedef __attribute__((address_space(3))) unsigned short lds_u16;
    const unsigned plane_bytes = (unsigned)HW * 2u;          // one bf16 plane
    const unsigned plane_bytes32 = (unsigned)HW * 4u;        // one fp32 / int32 plane (grid, idx)
    // ---- tap descriptors: one LDS byte address + two fractions per pixel, two flag bits per pixel ----
    unsigned ta[QP][4];
    float tf[QP][4][2];
    unsigned oob = 0;                                        // bit 2 p: east column outside, bit 2 p + 1: south row outside (p = 4 j + m)
    {
        const unsigned img_lds = (unsigned)(size_t)sImg;
#pragma unroll
        for (int j = 0; j < QP; ++j)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const TapsLite t = make_taps_lite(gx[j][m], gy[j][m], H, W);
                if constexpr (AUX) {
                    if (P.grid && live)
                        *reinterpret_cast<float2*>(reinterpret_cast<char*>(P.grid) + (size_t)b * 2 * plane_bytes32 + 8u * pixel_idx(j, m)) =
                            make_float2(gx[j][m], gy[j][m]);
                    if (P.idx && live)
                        *reinterpret_cast<int2*>(reinterpret_cast<char*>(P.idx) + (size_t)b * 2 * plane_bytes32 + 8u * pixel_idx(j, m)) =
                            make_int2(t.x0, t.y0);
                }
                ta[j][m] = img_lds + 2u * (unsigned)t.o00;
                tf[j][m][0] = t.wx; tf[j][m][1] = t.wy;      // the four weights are re-formed from these at the taps
                oob |= (t.inx ? 0u : 1u) << (2 * (4 * j + m));
                oob |= (t.iny ? 0u : 2u) << (2 * (4 * j + m));
            }
#pragma unroll
        for (int j = 0; j < QP; ++j)
#pragma unroll
            for (int m = 0; m < 4; ++m) asm volatile("" : "+v"(tf[j][m][0]), "+v"(tf[j][m][1]), "+v"(ta[j][m]));
        asm volatile("" : "+v"(oob));
    }

    wait_flag_lds(sFlag + 1, NLOAD);                         // the image has landed
    // the four taps of every channel: row 0 at a, row 1 at a + 2 W, channel planes 2 HW apart; a tap outside the image is
    // read anyway (the half-word exists: next row, next plane or the pad) and replaced by zero
    unsigned resp[QP][2][C];                                 // results, rounded: (west, east) mirror pixels of a channel per register
    const bool any_oob = __builtin_amdgcn_ballot_w64(oob != 0u) != 0;
    static_for<QP * 2>([&](auto jc) {
        constexpr int j = decltype(jc)::value / 2, mb0 = (decltype(jc)::value % 2) * 2;
        unsigned tv[2][C][4];
#pragma unroll
        for (int mm = 0; mm < 2; ++mm) {
            unsigned a0 = ta[j][mb0 + mm];
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                lds_cu16* p0 = (lds_cu16*)(size_t)a0;
                lds_cu16* p1 = (lds_cu16*)(size_t)(a0 + 2u * (unsigned)W);
                tv[mm][ch][0] = p0[0];
                tv[mm][ch][1] = p0[1];
                tv[mm][ch][2] = p1[0];
                tv[mm][ch][3] = p1[1];
                a0 += plane_bytes;
            }
        }
        auto combine = [&](auto oobc) {
            constexpr bool OOB = decltype(oobc)::value;
            float r2[2][C];
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                const int m = mb0 + mm;
                const unsigned fl = oob >> (2 * (4 * j + m));
                const bool inx = !(fl & 1u), iny = !(fl & 2u), inxy = !(fl & 3u);
                const float w = tf[j][m][0], nn = tf[j][m][1];
                const float e = 1.0f - w, s = 1.0f - nn;
                const float nw = s * e, ne = s * w, sw = nn * e, se = nn * w;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const float v00 = __uint_as_float(tv[mm][ch][0] << 16);
                    const float v01 = (!OOB || inx) ? __uint_as_float(tv[mm][ch][1] << 16) : 0.0f;
                    const float v10 = (!OOB || iny) ? __uint_as_float(tv[mm][ch][2] << 16) : 0.0f;
                    const float v11 = (!OOB || inxy) ? __uint_as_float(tv[mm][ch][3] << 16) : 0.0f;
                    float acc = v00 * nw;
                    acc = fmaf(v01, ne, acc);
                    acc = fmaf(v10, sw, acc);
                    acc = fmaf(v11, se, acc);
                    r2[mm][ch] = acc;
                }
            }
#pragma unroll
            for (int ch = 0; ch < C; ++ch) resp[j][mb0 / 2][ch] = pack_bf16(r2[0][ch], r2[1][ch]);   // the one rounding
        };
        if (any_oob) combine(std::true_type{}); else combine(std::false_type{});
    });
    lds_only_barrier();                                      // every tap of the image is in registers: its planes are free
    // results in place of the image, in the output's own layout (C, H, W), two pixels per word
#pragma unroll
    for (int j = 0; j < QP; ++j)
#pragma unroll
        for (int mh = 0; mh < 2; ++mh) {
            const unsigned pw = 2u * pixel_idx(j, 2 * mh), pe = 2u * pixel_idx(j, 2 * mh + 1);
            if (live) {
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    const unsigned x = resp[j][mh][ch];
                    *(lds_u16*)(size_t)((unsigned)(size_t)sImg + ch * plane_bytes + pw) = (unsigned short)(x & 0xffffu);
                    *(lds_u16*)(size_t)((unsigned)(size_t)sImg + ch * plane_bytes + pe) = (unsigned short)(x >> 16);
                }
            }
        }
    lds_only_barrier();                                      // results staged

    // copy-out: this band's rows [ra, ra + rows) and their mirror rows of every channel, 16 bytes (8 pixels) per lane
    // (the launcher guarantees rows W % 8 == 0)
    const int rows = (P.RGB / P.bands) * QP * BH;
    const int ra = band * rows;
    const int seg16 = (rows * W) >> 3;                       // 16-byte pieces of one row range of one plane
    const int nct = NW * kWave;
    gchar* ob = (gchar*)(P.out) + (size_t)b * C * plane_bytes;
    if (P.bands == 1) {
        // one workgroup owns the image: upper and lower row ranges of every plane are one contiguous run (no division)
        for (int e = tid; e < 2 * C * seg16; e += nct) {
            const v4f x = *reinterpret_cast<const v4f*>(sImg + 16u * (unsigned)e);
            store16_nt(ob + 16u * (unsigned)e, x);
        }
        return;
    }
    for (int e = tid; e < 2 * C * seg16; e += nct) {
        const int sg = e / seg16, i = e - sg * seg16;        // segment = (channel, upper / lower range)
        const int ch = sg >> 1;
        const int row_lo = (sg & 1) ? H - ra - rows : ra;
        const unsigned off = (unsigned)ch * plane_bytes + 2u * (unsigned)(row_lo * W) + 16u * (unsigned)i;
        const v4f x = *reinterpret_cast<const v4f*>(sImg + off);
        store16_nt(ob + off, x);
    }
}

}  // namespace tpspp_geo
