// Device-side primitives shared by the kernel files: the wavefront width, the vector types of the MFMA operands, bf16
// rounding and packing, the transposing LDS read, lane reads and the butterfly reductions.  Each stands here once; a
// kernel file keeps a helper of its own only where its arithmetic differs (tpspp_dgab.hip's DPP reductions, the GELUs).
// Everything is __forceinline__: the kernels' register budgets were tuned with these bodies inlined.
#pragma once
#include <hip/hip_runtime.h>

namespace tpspp_dev {

constexpr int kWave = 64;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// fp32 -> bf16 bits, round to nearest even in integer arithmetic (inputs are finite activations)
__device__ __forceinline__ unsigned f32_to_bf16_bits(float f)
{
    unsigned u = __builtin_bit_cast(unsigned, f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h)
{
    return __builtin_bit_cast(float, (unsigned)h << 16);
}

// v_cvt_pk_bf16_f32: two fp32 -> packed bf16, round to nearest even
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    f32x2 v; v[0] = lo; v[1] = hi;
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// hi / lo halves of a pair for the three-term bf16 split: hi = bf16(v), lo = bf16(v - hi)
__device__ __forceinline__ void split2(float v0, float v1, unsigned& hi, unsigned& lo)
{
    hi = pack_bf16(v0, v1);
    const float h0 = __builtin_bit_cast(float, hi << 16), h1 = __builtin_bit_cast(float, hi & 0xffff0000u);
    lo = pack_bf16(v0 - h0, v1 - h1);
}

// v_mfma_f32_16x16x32_bf16 on operands held as four 32-bit words of packed bf16
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ds_read_b64_tr_b16: lane (l & 15) of a 16-lane group gets column l & 15 of a [4 rows][16 columns] block of 16-bit
// elements whose rows the lanes point at
__device__ __forceinline__ u32x2 read_tr(const unsigned short* p)
{
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p));
}

__device__ __forceinline__ float readlane_f(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// __shfl_xor butterfly over the wavefront: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// deterministic sums over the 256 threads of a workgroup (butterfly within the wavefront, then the four wavefronts in
// order); red: K x 4 floats of LDS.  Every thread ends with the same bits.
template <int K>
__device__ __forceinline__ void block_sums(float (&v)[K], float (*red)[4])
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
    __syncthreads();
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace tpspp_dev
