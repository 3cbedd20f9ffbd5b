// nn_optim.hip -- gfx950 kernels for the optimiser step of the SELD CRNN (C ABI: include/salsa_nn.h): Adam over all tensors in
// one launch, and the bf16 filter bank the hand-written convolutions read, rebuilt from the float32 master filters every step.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "../../include/salsa_nn.h"
#include "nn_common.h" // pack_bf16

namespace {

// ------------------------------------------------------------------------------------------------ convolution filter bank
// Every step the hand-written convolutions need each float32 master filter (Cout, Cin, 3, 3) as bf16 in two layouts: the
// forward kernel's [Cout][3][3][Cin] and the data-gradient kernel's flipped / transposed [Cin][3][3][Cout].  Through torch
// that was four small kernels per layer per step (cast, permute copy, flip, permute copy: 68 launches, ~0.5 ms); here ONE
// launch does all layers.  A block = one layer's 32 x 32 (co, ci) tile with its nine taps: the 32 x 288 floats go through LDS
// (row pitch 289: both read patterns below are bank-conflict-free) and leave as 64-byte runs in either layout.
// desc: 11 x int64 per layer = src, fwd, bwd pointers, Cout, Cin, element strides of src (co, ci, ky, kx), first block, taps
// (9, or 1 for the 1x1 shortcut filters: forward [Cout][Cin], data-gradient [Cin][Cout]).
__global__ __launch_bounds__(256) void conv_filter_bank_kernel(const long long *__restrict__ desc, int n_layers)
{
    __shared__ float tile[32][289];
    int l = 0;
    while (l + 1 < n_layers && (long long)blockIdx.x >= desc[(l + 1) * 11 + 9]) l++;
    const long long *d = desc + l * 11;
    const float *src = (const float *)d[0];
    __hip_bfloat16 *fwd = (__hip_bfloat16 *)d[1], *bwd = (__hip_bfloat16 *)d[2];
    const int Cout = (int)d[3], Cin = (int)d[4], taps = (int)d[10], rw = 32 * taps; // taps = 9 or 1
    const long s_co = d[5], s_ci = d[6], s_ky = d[7], s_kx = d[8];
    const int t = (int)(blockIdx.x - d[9]), tiles_ci = Cin / 32, co0 = (t / tiles_ci) * 32, ci0 = (t % tiles_ci) * 32;
    if (s_ci == 1 && !(s_co & 3) && !(s_ky & 3) && !(s_kx & 3)) { // channels-last master filter (the trainer's): 16-byte loads along ci
        for (int e = threadIdx.x; e < 8 * rw; e += 256) {
            const int co = e / (8 * taps), q = e % (8 * taps), ci = (q % 8) * 4, tap = q / 8;
            const float4 v = *(const float4 *)(src + (co0 + co) * s_co + (ci0 + ci) + (tap / 3) * s_ky + (tap % 3) * s_kx);
            tile[co][ci * taps + tap] = v.x;
            tile[co][(ci + 1) * taps + tap] = v.y;
            tile[co][(ci + 2) * taps + tap] = v.z;
            tile[co][(ci + 3) * taps + tap] = v.w;
        }
    } else {
        for (int e = threadIdx.x; e < 32 * rw; e += 256) { // consecutive threads walk the source's contiguous axis: ci when the
            // master filter is channels-last (s_ci == 1), the taps when it is torch's default (co, ci, ky, kx)
            const int co = e / rw, q = e % rw;
            const int ci = s_ci == 1 ? q % 32 : q / taps, tap = s_ci == 1 ? q / 32 : q % taps;
            tile[co][ci * taps + tap] = src[(co0 + co) * s_co + (ci0 + ci) * s_ci + (tap / 3) * s_ky + (tap % 3) * s_kx];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * rw; e += 256) { // two neighbouring channels per thread: 4-byte stores, 64-byte runs per 16 lanes
        const int a = (e % 16) * 2, tap = (e / 16) % taps, b = e / (16 * taps);
        *(unsigned *)(fwd + ((long)(co0 + b) * taps + tap) * Cin + ci0 + a) = pack_bf16(tile[b][a * taps + tap], tile[b][(a + 1) * taps + tap]); // (co = b, ci = a)
        if (bwd)
            *(unsigned *)(bwd + ((long)(ci0 + b) * taps + (taps - 1 - tap)) * Cout + co0 + a) = pack_bf16(tile[a][b * taps + tap], tile[a + 1][b * taps + tap]); // (ci = b, co = a)
    }
}

} // namespace

/* bf16 copies of all hand-written convolution layers' float32 filters in ONE launch: the forward layout [Cout][3][3][Cin] and
 * (when bwd != 0) the data-gradient layout [Cin][3][3][Cout] with the taps flipped.  desc (device): n_layers x 11 int64 =
 * {src, fwd, bwd, Cout, Cin, src element strides co / ci / ky / kx, first block, taps (9 | 1)}; layer l owns (Cout/32)*(Cin/32) blocks from
 * its first block on; n_blocks = their total.  Cout and Cin must be multiples of 32. */
extern "C" int salsa_nn_conv_filter_bank(const void *desc, int n_layers, int n_blocks, void *hip_stream)
{
    if (!desc || n_layers <= 0 || n_blocks <= 0) return -1;
    hipLaunchKernelGGL(conv_filter_bank_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)hip_stream, (const long long *)desc,
                       n_layers);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// ------------------------------------------------------------------------------------------------------------ Adam, one launch
namespace {
struct AdamGrads {
    const float *g[SALSA_NN_ADAM_MAX_TENSORS];
};
__global__ __launch_bounds__(256) void adam_step_kernel(const salsa_nn_adam_entry *__restrict__ table, const AdamGrads grads,
                                                        const int2 *__restrict__ chunks, float w1 /* 1 - beta1 */, float beta2,
                                                        float w2 /* 1 - beta2 */, float step_size, float bc2_sqrt, float eps, float wd)
{
    const int2 ch = chunks[blockIdx.x];
    const salsa_nn_adam_entry e = table[ch.x];
    const float *__restrict__ g = grads.g[ch.x];
    const long first = (long)ch.y * SALSA_NN_ADAM_CHUNK;
    const long last = first + SALSA_NN_ADAM_CHUNK < e.n ? first + SALSA_NN_ADAM_CHUNK : e.n;
    auto update = [&](float &p, float &m, float &v, float gr) {
        if (wd != 0.f) gr += p * wd;
        m = m + w1 * (gr - m);                       // lerp(m, g, 1 - beta1), weight < 0.5
        v = beta2 * v + w2 * gr * gr;
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p -= step_size * m / denom;
    };
    const bool vec = ((((uintptr_t)e.p | (uintptr_t)e.m | (uintptr_t)e.v | (uintptr_t)g) & 15) == 0) && (e.n & 3) == 0;
    if (vec) {
        for (long i = first + 4 * threadIdx.x; i < last; i += 4 * 256) {
            float4 p = *(float4 *)(e.p + i), m = *(float4 *)(e.m + i), v = *(float4 *)(e.v + i);
            const float4 gr = *(const float4 *)(g + i);
            update(p.x, m.x, v.x, gr.x); update(p.y, m.y, v.y, gr.y); update(p.z, m.z, v.z, gr.z); update(p.w, m.w, v.w, gr.w);
            *(float4 *)(e.p + i) = p; *(float4 *)(e.m + i) = m; *(float4 *)(e.v + i) = v;
        }
    } else {
        for (long i = first + threadIdx.x; i < last; i += 256) update(e.p[i], e.m[i], e.v[i], g[i]);
    }
}
} // namespace

extern "C" int salsa_nn_adam_step(const salsa_nn_adam_entry *table, const float *const *grads, int n_tensors, const int *chunks, int n_chunks,
                                  double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *hip_stream)
{
    if (!table || !grads || !chunks || n_tensors <= 0 || n_tensors > SALSA_NN_ADAM_MAX_TENSORS || n_chunks <= 0 || step < 1) return -1;
    AdamGrads ga;
    for (int i = 0; i < n_tensors; i++) {
        if (!grads[i]) return -1;
        ga.g[i] = grads[i];
    }
    for (int i = n_tensors; i < SALSA_NN_ADAM_MAX_TENSORS; i++) ga.g[i] = nullptr;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)hip_stream, table, ga, (const int2 *)chunks,
                       (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps,
                       (float)weight_decay); // (the hyper-parameters combine in double, as torch's kernel does per element)
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
