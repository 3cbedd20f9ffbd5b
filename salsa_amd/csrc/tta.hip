// tta.hip -- salsa_nn_tta_variant and salsa_nn_tta_merge (include/salsa_nn.h): the two device steps of test-time augmentation and
// model ensembling around the CRNN forward.  The arithmetic is tta.h's.
//
//   tta_variant_kernel<W>  one thread = W consecutive elements of ALL channels of one sample: loads, the channel swap of variant v
//                          (bank_batch::swap7, or the GCC gather with its lag flip), stores.  W = 4 when every access is a 16-byte one
//                          (the channel planes and strides are multiples of four elements and both pointers are 16-byte aligned; GCC:
//                          F a multiple of four too, so a flipped group is one aligned load read back to front); any other shape runs
//                          W = 1.  A plane of the dense output must START aligned, so W = 4 needs T F % 4 == 0 and has no tail.
//                          Pure streaming: every input element is read once per output element it feeds.
//   tta_merge_kernel       one thread = one (clip, label frame, class): its N outputs read from the slabs, un-swapped, added in a
//                          fixed order and divided once.  No atomics, no LDS: bit-reproducible.
// Both are asynchronous on the caller's stream, allocate nothing and synchronise nothing.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "tta.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

template <int W>
__global__ __launch_bounds__(256) void tta_variant_kernel(const float *__restrict__ in, int64_t in_batch, int64_t in_chan,
                                                          float *__restrict__ out, int T, int F, int kind, int v)
{
    const int b = blockIdx.y;
    const int64_t plane = (int64_t)T * F;
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (e >= plane) return;                                                 // (W = 4: plane % 4 == 0, so e + 3 < plane as well)
    int m[4];
    tta::variant_bits(kind, v, m);
    const float *src = in + (int64_t)b * in_batch;
    if (kind == tta::KIND_GCC) {
        const int t = (int)(e / F), f = (int)(e - (int64_t)t * F);         // (W = 4: F % 4 == 0, the group stays inside frame t)
        tta::variant10<W>(src, in_chan, out + (int64_t)b * 10 * plane, plane, t, f, F, v);
    } else {
        tta::variant7<W>(src, in_chan, out + (int64_t)b * 7 * plane, plane, e, kind == tta::KIND_MIC, m);
    }
}

__global__ __launch_bounds__(256) void tta_merge_kernel(const float *__restrict__ prob, const float *__restrict__ xyz, int n_models,
                                                        const tta::ids_t ids, int n_var, int kind, int64_t cells, int nc,
                                                        float *__restrict__ prob_out, float *__restrict__ xyz_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells * nc) return;
    const int64_t cell = i / nc;
    const int k = (int)(i - cell * nc);
    float o[4];
    tta::merge_one(prob, xyz, n_models, ids, n_var, kind, cells, nc, cell, k, o);
    prob_out[i] = o[0];
    float *d = xyz_out + cell * 3 * nc + k;
    d[0] = o[1];
    d[nc] = o[2];
    d[2 * nc] = o[3];
}

int tfail(int code, const char *msg)
{
    salsa_set_last_error_(msg);
    return code;
}

} // namespace

extern "C" int salsa_nn_tta_variant(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch,
                                    int n_frames, int n_freq, int kind, int v, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    const int V = tta::n_variants(kind);
    if (!V) return tfail(-1, "salsa_nn_tta_variant: unknown kind (1 foa, 2 mic, 3 gcc)");
    if (v < 0 || v >= V) return tfail(-1, "salsa_nn_tta_variant: variant id outside [0, V)");
    if (!d_in || !d_out || d_in == d_out) return tfail(-1, "salsa_nn_tta_variant: NULL input or output, or an in-place call");
    if (batch <= 0 || batch > 65535 || n_frames <= 0 || n_freq <= 0 || (int64_t)n_frames * n_freq >= INT32_MAX)
        return tfail(-1, "salsa_nn_tta_variant: bad batch, frame or bin count");
    const int C = kind == tta::KIND_GCC ? 10 : 7;
    const int64_t plane = (int64_t)n_frames * n_freq;
    if (in_channel_stride < plane || in_batch_stride < C * in_channel_stride || in_batch_stride > INT64_MAX / 4 / 65536)
        return tfail(-1, "salsa_nn_tta_variant: input strides smaller than the [C][T][F] block");
    const bool wide = plane % 4 == 0 && in_channel_stride % 4 == 0 && in_batch_stride % 4 == 0 && !((uintptr_t)d_in & 15) &&
                      !((uintptr_t)d_out & 15) && (kind != tta::KIND_GCC || n_freq % 4 == 0);
    hipStream_t st = (hipStream_t)hip_stream;
    if (wide)
        hipLaunchKernelGGL(tta_variant_kernel<4>, dim3((unsigned)((plane / 4 + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_in,
                           in_batch_stride, in_channel_stride, d_out, n_frames, n_freq, kind, v);
    else
        hipLaunchKernelGGL(tta_variant_kernel<1>, dim3((unsigned)((plane + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_in,
                           in_batch_stride, in_channel_stride, d_out, n_frames, n_freq, kind, v);
    if (hipGetLastError() != hipSuccess) return tfail(-6, "salsa_nn_tta_variant: launch failed");
    return 0;
}

extern "C" int salsa_nn_tta_merge(const float *d_prob_slab, const float *d_xyz_slab, int n_models, const int *variant_ids,
                                  int n_variants, int kind, int batch, int label_frames, int n_classes, float *d_prob_out,
                                  float *d_xyz_out, void *hip_stream)
{
    const int V = tta::n_variants(kind);
    if (!V) return tfail(-1, "salsa_nn_tta_merge: unknown kind (1 foa, 2 mic, 3 gcc)");
    if (!d_prob_slab || !d_xyz_slab || !variant_ids || !d_prob_out || !d_xyz_out)
        return tfail(-1, "salsa_nn_tta_merge: NULL slab, variant list or output");
    if (n_models < 1 || n_variants < 1 || n_variants > tta::MAX_VARIANTS || n_models > 4096)
        return tfail(-1, "salsa_nn_tta_merge: N = n_models x n_variants must be at least 1 (at most 16 variants, 4096 models)");
    tta::ids_t ids = {};
    for (int i = 0; i < n_variants; i++) {
        if (variant_ids[i] < 0 || variant_ids[i] >= V) return tfail(-1, "salsa_nn_tta_merge: variant id outside [0, V)");
        ids.v[i] = variant_ids[i];
    }
    if (batch < 1 || label_frames < 1 || n_classes < 1 || (int64_t)batch * label_frames * n_classes >= INT32_MAX / 4)
        return tfail(-1, "salsa_nn_tta_merge: bad batch, label frame or class count");
    const int64_t cells = (int64_t)batch * label_frames, n = cells * n_classes;
    hipLaunchKernelGGL(tta_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, d_prob_slab,
                       d_xyz_slab, n_models, ids, n_variants, kind, cells, n_classes, d_prob_out, d_xyz_out);
    if (hipGetLastError() != hipSuccess) return tfail(-6, "salsa_nn_tta_merge: launch failed");
    return 0;
}
