// Launcher of the bf16 classic warp kernel (tpspp_warp_geo_bf16.h): geometry planning + the (C, QP, AUX) instantiations.
// Its own translation unit, compiled like tpspp_warp_geo.hip with -fno-slp-vectorize (tps_pp_amd/build.py): the grid chains
// are the same code and packed fp32 FMAs are slower here.
#include "tpspp_common.h"
#include "tpspp_warp_geo_bf16.h"
#include "tpspp_warp_geo_launch.h"

namespace tpspp {

using tpspp_dev::kWave;

namespace {

struct Plan16 { int QP, BW, CG, RGB, bands, nthr, NW, nload; size_t lds; };

// The decomposition of tpspp_warp_geo.hip's plan_geo for one image per workgroup: the table's QP (the packed table is
// shared with the fp32 kernels), the fewest bands whose workgroup fits the wavefront budget, one loader per ~40 KB.
bool plan_geo16(int C, int H, int W, int F, Plan16* p, const char** why)
{
    if (!(C == 1 || C == 3)) { *why = "C0 must be 1 or 3"; return false; }
    if (F != 20) { *why = "F must be 20"; return false; }
    const int QP = geo_qp(H, W);
    if (QP == 0 || (H * W) % 8 != 0) { *why = "no prepared table for this geometry (Ho % 16 == 0, Wo % 4 == 0)"; return false; }
    p->QP = QP;
    p->BW = tpspp_img::img_block_w(W);
    const int BH = 32 / p->BW;
    p->CG = ((W / 2) + p->BW - 1) / p->BW;
    p->RGB = ((H / 2) / BH) / QP;
    p->lds = tpspp_geo16::geo16_lds_bytes(F + 3, C, H, W);
    if (p->lds > 160 * 1024) { *why = "the bf16 image does not fit the LDS (160 KB)"; return false; }
    p->nload = (int)((size_t)C * H * W * 2 / (40 * 1024)) + 1;
    if (p->nload > 3) p->nload = 3;
    const int max_waves = QP >= 3 ? 12 : 16;
    for (int B = 1; B <= p->RGB; ++B) {
        if (p->RGB % B) continue;
        const int nthr = p->CG * (p->RGB / B) * 32;
        const int NW = (nthr + kWave - 1) / kWave;
        const int rows = (p->RGB / B) * QP * BH;
        if ((rows * W) % 8 != 0) continue;                   // a band's row range leaves in whole 16-byte pieces
        if (NW + p->nload <= max_waves && NW <= 13) { p->bands = B; p->nthr = nthr; p->NW = NW; return true; }
    }
    *why = "no decomposition of the quadrant into workgroups";
    return false;
}

template <int C, int QP, bool AUX>
void launch_one16(const tpspp_geo16::Geo16Params& P, const Plan16& pl, hipStream_t st)
{
    auto kern = tpspp_geo16::tps_warp_geo_bf16_kernel<20, C, QP, AUX>;
    static bool attr_done[kMaxDevices] = {};
    if (first_use_on_device(attr_done)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)P.N * (unsigned)pl.bands), dim3((unsigned)((pl.NW + pl.nload) * kWave)), pl.lds, st, P);
}

template <int C, int QP>
void launch_aux16(const tpspp_geo16::Geo16Params& P, const Plan16& pl, hipStream_t st)
{
    if (P.grid || P.idx) launch_one16<C, QP, true>(P, pl, st);
    else launch_one16<C, QP, false>(P, pl, st);
}

template <int C>
void launch_qp16(const tpspp_geo16::Geo16Params& P, const Plan16& pl, hipStream_t st)
{
    switch (pl.QP) {
    case 1: launch_aux16<C, 1>(P, pl, st); break;
    case 2: launch_aux16<C, 2>(P, pl, st); break;
    case 3: launch_aux16<C, 3>(P, pl, st); break;
    default: launch_aux16<C, 4>(P, pl, st); break;
    }
}

}  // namespace

const char* geo_bf16_kernel_refusal(int C, int H, int W, int F)
{
    Plan16 pl;
    const char* why = nullptr;
    return plan_geo16(C, H, W, F, &pl, &why) ? nullptr : why;
}

bool launch_geo_bf16_kernel(int C, int H, int W, int F, const void* in, const float* ctrl, const float* inv_delta_c,
                            const float* packed, int N, void* out, float* grid, int32_t* idx, hipStream_t st)
{
    Plan16 pl;
    const char* why = nullptr;
    if (!plan_geo16(C, H, W, F, &pl, &why)) return false;
    tpspp_geo16::Geo16Params P;
    P.in = static_cast<const unsigned short*>(in); P.ctrl = ctrl; P.inv_delta_c = inv_delta_c; P.packed = packed; P.N = N;
    P.out = static_cast<unsigned short*>(out); P.grid = grid; P.idx = idx;
    P.H = H; P.W = W; P.BW = pl.BW; P.CG = pl.CG; P.RGB = pl.RGB; P.bands = pl.bands; P.nthr = pl.nthr; P.NW = pl.NW;
    P.img_off = tpspp_geo::geo_img_off(F + 3, 1);
    if (C == 1) launch_qp16<1>(P, pl, st);
    else launch_qp16<3>(P, pl, st);
    return true;
}

}  // namespace tpspp
