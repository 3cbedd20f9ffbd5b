// nn_vec.h -- internal: the 16-byte vector access of the streaming passes (nn_pool.hip, nn_batchnorm.hip): one thread = L channels
// of one pixel, channels-last, as float32 x 4 or bf16 x 8.  (This bf16x8 is a struct of eight shorts, conv_internal.h's a __bf16
// vector: no unit includes both.)
#pragma once
#include <hip/hip_runtime.h>
#include "nn_common.h" // pack_bf16

namespace {

struct f32x4 {
    float v[4];
};
struct bf16x8 {
    unsigned short v[8];
};

__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

// Round-5 probes: the 16-byte vector loads / stores of the streaming passes (BatchNorm, pooling) as non-temporal accesses
// (-DNN_NT_LD=1 / -DNN_NT_ST=1).  Every tensor these passes touch is read or written exactly once per launch.
#ifndef NN_NT_LD
#define NN_NT_LD 0
#endif
#ifndef NN_NT_ST
#define NN_NT_ST 0
#endif
typedef unsigned nn_u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 nn_ld16(const void *p)
{
    if (NN_NT_LD) {
        const nn_u4v t = __builtin_nontemporal_load((const nn_u4v *)p);
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    return *(const uint4 *)p;
}
__device__ __forceinline__ void nn_st16(void *p, const uint4 v)
{
    if (NN_NT_ST) {
        const nn_u4v t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, (nn_u4v *)p);
    } else
        *(uint4 *)p = v;
}

template <typename V, int L> struct vec_io;
template <> struct vec_io<f32x4, 4> {
    typedef float4 raw_t;
    static __device__ __forceinline__ raw_t load_raw(const void *p) { return *(const float4 *)p; }
    static __device__ __forceinline__ void convert(const raw_t &t, float *f) { f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w; }
    static __device__ __forceinline__ void load(const void *p, float *f)
    {
        const float4 t = *(const float4 *)p;
        f[0] = t.x; f[1] = t.y; f[2] = t.z; f[3] = t.w;
    }
    static __device__ __forceinline__ void store(void *p, const float *f) { *(float4 *)p = make_float4(f[0], f[1], f[2], f[3]); }
};
template <> struct vec_io<bf16x8, 8> {
    typedef uint4 raw_t;
    static __device__ __forceinline__ raw_t load_raw(const void *p) { return nn_ld16(p); }
    static __device__ __forceinline__ void convert(const raw_t &t, float *f)
    {
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            f[2 * i] = bf2f((unsigned short)(w[i] & 0xffffu));
            f[2 * i + 1] = bf2f((unsigned short)(w[i] >> 16));
        }
    }
    static __device__ __forceinline__ void load(const void *p, float *f) { convert(load_raw(p), f); }
    static __device__ __forceinline__ void store(void *p, const float *f)
    {
        unsigned w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = pack_bf16(f[2 * i], f[2 * i + 1]);
        nn_st16(p, make_uint4(w[0], w[1], w[2], w[3]));
    }
};

} // namespace

// launches KERNEL<vector type, L> for the caller's `dtype` (1 = bf16) on its stream `st`
#define NN_LAUNCH(KERNEL, grid, block, ...)                                                               \
    do {                                                                                                  \
        if (dtype == 1) hipLaunchKernelGGL((KERNEL<bf16x8, 8>), grid, block, 0, st, __VA_ARGS__);          \
        else hipLaunchKernelGGL((KERNEL<f32x4, 4>), grid, block, 0, st, __VA_ARGS__);                      \
    } while (0)
