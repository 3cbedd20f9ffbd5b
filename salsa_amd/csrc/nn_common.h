// nn_common.h -- internal: what the BatchNorm kernels (nn_batchnorm.hip) and the convolutions that apply a BatchNorm on the fly while
// staging their input (conv_mfma.hip, conv_c64_wrw.hip, round 4) must agree on bit for bit: the counter-based dropout mask, and
// the float32 -> bf16 rounding of every kernel that stores bf16 (the one header both nn_vec.h and conv_internal.h include).
#pragma once
#include <hip/hip_runtime.h>
namespace {
// two float32 -> packed bf16 (low half = a), round to nearest even: one v_cvt_pk_bf16_f32 on gfx950
__device__ __forceinline__ unsigned pack_bf16(float a, float b)
{
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{a, b}, bf16x2_t));
}
struct DropArgs {
    unsigned thresh; // drop when the element's 16 bits < thresh ; 0 = no dropout
    unsigned seed;
    float scale;     // 65536 / (65536 - thresh)
};
__device__ inline unsigned drop_hash(unsigned pair, unsigned seed)
{
    unsigned h = pair * 0x9E3779B1u + seed;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
static inline DropArgs drop_args(float p, unsigned seed)
{
    DropArgs d = {0u, seed, 1.f};
    if (p > 0.f) {
        d.thresh = (unsigned)(p * 65536.f + 0.5f);
        if (d.thresh > 65535u) d.thresh = 65535u;
        d.scale = 65536.f / (float)(65536u - d.thresh);
    }
    return d;
}
} // namespace
