// track_align.hip -- salsa_nn_tta_merge_multi and salsa_nn_chunk_merge_multi (include/salsa_nn.h): merging the Multi-ACCDOA outputs of
// several forwards of one clip -- test-time augmentation, ensembles, overlapping test chunks -- after their tracks are aligned cell by
// cell.  The arithmetic is track_align.h's.
//
// Both kernels: one thread per (row, real class) item with the class index fastest, salsa_nn_adpit_loss's mapping.  An item reads
// the 9 vector components of its cell C columns apart, so the lanes of a wave that share a row read 9 runs of consecutive floats that
// together are the row's 9 C columns: every fetched line is used in full, and a row's second visit (the next component) hits the
// line the first one brought in.  The cell, the anchor and the sums stay in registers (the permutation is applied by selection, not
// by indexing), no LDS, no atomics, no scratch buffer: an item's result depends on that item's inputs alone, so it is bit-reproducible
// and a clip's result does not depend on its batch.  Both are asynchronous on the caller's stream and allocate nothing.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "track_align.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void tta_merge_multi_kernel(const float *__restrict__ xyz, int n_models, const tta::ids_t ids,
                                                                  int n_var, int kind, int64_t cells, int C, float *__restrict__ act_out,
                                                                  float *__restrict__ xyz_out, int *__restrict__ perm)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= cells * C) return;
    const int64_t cell = i / C;
    const int c = (int)(i - cell * C);
    float v[9], a[3];
    track_align::merge_cell(xyz, n_models, ids, n_var, kind, cells, C, cell, c, v, a, perm);
    float *pa = act_out + cell * 3 * C + c, *pv = xyz_out + cell * 9 * C + c;
#pragma unroll
    for (int n = 0; n < 3; n++) {
        pa[(int64_t)n * C] = a[n];
#pragma unroll
        for (int k = 0; k < 3; k++) pv[(int64_t)(3 * k + n) * C] = v[n * 3 + k];
    }
}

__global__ __launch_bounds__(THREADS) void chunk_merge_multi_kernel(const float *__restrict__ act, const float *__restrict__ xyz,
                                                                    int64_t n_items, int n_chunks, int chunk_len, int chunk_hop,
                                                                    int n_frames, int C, float *__restrict__ file_act,
                                                                    float *__restrict__ file_xyz)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_items) return;
    const int64_t row = i / C;                                              // file * n_frames + frame
    const int c = (int)(i - row * C);
    const int64_t file = row / n_frames;
    const int frame = (int)(row - file * n_frames);
    const int64_t chunk_rows = (int64_t)n_chunks * chunk_len;
    float v[9], a[3];
    track_align::file_cell(act + file * chunk_rows * 3 * C, xyz + file * chunk_rows * 9 * C, n_chunks, chunk_len, chunk_hop, n_frames, C,
                           frame, c, a, v);
    float *pa = file_act + row * 3 * C + c, *pv = file_xyz + row * 9 * C + c;
#pragma unroll
    for (int n = 0; n < 3; n++) {
        pa[(int64_t)n * C] = a[n];
#pragma unroll
        for (int k = 0; k < 3; k++) pv[(int64_t)(3 * k + n) * C] = v[n * 3 + k];
    }
}

int afail(const char *msg)
{
    salsa_set_last_error_(msg);
    return -1;
}

} // namespace

extern "C" int salsa_nn_tta_merge_multi(const float *d_xyz_slab, int n_models, const int *variant_ids, int n_variants, int kind, int batch,
                                        int label_frames, int n_real_classes, float *d_xyz_out, float *d_act_out, int *d_perm_out,
                                        void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    const int V = tta::n_variants(kind);
    if (!V) return afail("salsa_nn_tta_merge_multi: unknown kind (1 foa, 2 mic, 3 gcc)");
    if (!d_xyz_slab || !variant_ids || !d_xyz_out || !d_act_out) return afail("salsa_nn_tta_merge_multi: NULL slab, variant list or output");
    if (n_models < 1 || n_variants < 1 || n_variants > tta::MAX_VARIANTS || n_models > 4096)
        return afail("salsa_nn_tta_merge_multi: N = n_models x n_variants must be at least 1 (at most 16 variants, 4096 models)");
    tta::ids_t ids = {};
    for (int i = 0; i < n_variants; i++) {
        if (variant_ids[i] < 0 || variant_ids[i] >= V) return afail("salsa_nn_tta_merge_multi: variant id outside [0, V)");
        ids.v[i] = variant_ids[i];
    }
    if (batch < 1 || label_frames < 1 || n_real_classes < 1 || (int64_t)batch * label_frames >= INT32_MAX ||
        (int64_t)batch * label_frames * 9 * n_real_classes >= INT32_MAX / ((int64_t)n_models * n_variants))
        return afail("salsa_nn_tta_merge_multi: bad batch, label frame or class count (the slab is indexed in int32)");
    const int64_t cells = (int64_t)batch * label_frames, n = cells * n_real_classes;
    hipLaunchKernelGGL(tta_merge_multi_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)hip_stream,
                       d_xyz_slab, n_models, ids, n_variants, kind, cells, n_real_classes, d_act_out, d_xyz_out, d_perm_out);
    if (hipGetLastError() != hipSuccess) {
        salsa_set_last_error_("salsa_nn_tta_merge_multi: launch failed");
        return -6;
    }
    return 0;
}

extern "C" int salsa_nn_chunk_merge_multi(const float *d_act, const float *d_xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop,
                                          int n_frames, int n_real_classes, float *d_file_act, float *d_file_xyz, void *hip_stream)
{
    if (!d_act || !d_xyz || !d_file_act || !d_file_xyz) return afail("salsa_nn_chunk_merge_multi: NULL input or output");
    if (n_files < 1 || n_chunks < 1 || n_frames < 1 || n_real_classes < 1 || chunk_len < 1 || chunk_hop < 1)
        return afail("salsa_nn_chunk_merge_multi: a count below 1");
    if ((int64_t)n_chunks * chunk_len >= INT32_MAX || (int64_t)n_files * n_chunks * chunk_len * 9 * n_real_classes >= INT32_MAX ||
        (int64_t)n_files * n_frames * 9 * n_real_classes >= INT32_MAX)
        return afail("salsa_nn_chunk_merge_multi: the chunks or the file outputs are beyond int32 indexing");
    if (n_chunks > 1 && (chunk_hop > chunk_len || chunk_len > n_frames))
        return afail("salsa_nn_chunk_merge_multi: chunk_hop > chunk_len or chunk_len > n_frames with more than one chunk");
    if (n_chunks != seld_decode::expected_chunks(n_frames, chunk_len, chunk_hop))
        return afail("salsa_nn_chunk_merge_multi: n_chunks is not the number of chunk starts");
    const int64_t n = (int64_t)n_files * n_frames * n_real_classes;
    hipLaunchKernelGGL(chunk_merge_multi_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)hip_stream,
                       d_act, d_xyz, n, n_chunks, chunk_len, chunk_hop, n_frames, n_real_classes, d_file_act, d_file_xyz);
    if (hipGetLastError() != hipSuccess) {
        salsa_set_last_error_("salsa_nn_chunk_merge_multi: launch failed");
        return -6;
    }
    return 0;
}
