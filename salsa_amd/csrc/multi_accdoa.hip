// multi_accdoa.hip -- the Multi-ACCDOA output format on the device (include/salsa_nn.h; statements in
// multi_accdoa.h): salsa_nn_adpit_loss, the ADPIT training loss with its gradient, and salsa_nn_seld_decode_multi, the DCASE rows of
// a batch of files with near-identical tracks of one class unified.
//
// Loss: one thread per (row, class) item, grid-stride over 64 workgroups of 256; the item's 9 predictions, 3 slot activities and 9
// slot targets are read with the class index fastest (coalesced over a row), the gradient needs no sum and is written at once, and
// the item losses go into one float64 partial per workgroup that a one-thread finish launch adds in a fixed order (as
// salsa_nn_accdoa_loss does): bit-reproducible.
//
// Decode: one workgroup of 256 threads per file, tiles of 256 CONSECUTIVE (frame, class) cells as in seld_decode.hip.  A cell emits
// 0 .. 3 rows, so a lane's rank within its wave is a prefix sum of counts: two ballots (bit 0 and bit 1 of the count) and two
// popcounts of the lower lanes' bits; wave totals go through LDS and a running base carries earlier tiles.  No atomics, 8-byte row
// stores, rows sorted by (frame, class, group).
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "multi_accdoa.h"
#include "seld_rows.h" // DcaseRow

namespace {

constexpr int ADPIT_BLOCKS = SALSA_ADPIT_LOSS_WS, ADPIT_THREADS = 256;

__global__ __launch_bounds__(ADPIT_THREADS) void adpit_loss_partial_kernel(const float *__restrict__ doa, const float *__restrict__ sed_gt,
                                                                           const float *__restrict__ doa_gt, long rows, int C,
                                                                           float *__restrict__ g_logit, float *__restrict__ g_doa,
                                                                           uint8_t *__restrict__ chosen,
                                                                           double *__restrict__ partial /* [ADPIT_BLOCKS] */)
{
    __shared__ double red[ADPIT_THREADS];
    const long n = rows * C;
    const double denom = 9.0 * (double)n;                                    // 9 rows C < 2^53: exact
    double s = 0.0;
    for (long i = (long)blockIdx.x * ADPIT_THREADS + threadIdx.x; i < n; i += (long)ADPIT_BLOCKS * ADPIT_THREADS) {
        const long r = i / C;
        const int c = (int)(i - r * C);
        const long sed0 = r * 3 * C + c, doa0 = r * 9 * C + c;                // slot m: + m C; axis a, track n: + (3 a + n) C
        float P[9], T[9], sv[3], g[9];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            sv[m] = sed_gt[sed0 + (long)m * C];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                P[m * 3 + a] = doa[doa0 + (long)(3 * a + m) * C];
                T[m * 3 + a] = doa_gt[doa0 + (long)(3 * a + m) * C];
            }
        }
        double item;
        const int cand = multi_accdoa::adpit_item(P, sv, T, denom, &item, g);
        s += item;
#pragma unroll
        for (int m = 0; m < 3; m++) {
            if (g_logit) g_logit[sed0 + (long)m * C] = 0.f;
#pragma unroll
            for (int a = 0; a < 3; a++) g_doa[doa0 + (long)(3 * a + m) * C] = g[m * 3 + a];
        }
        if (chosen) chosen[i] = (uint8_t)cand;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = ADPIT_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void adpit_loss_finish_kernel(const double *__restrict__ partial, long rows, int C,
                                                               float *__restrict__ out3)
{
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int b = 0; b < ADPIT_BLOCKS; b++) t += partial[b];
    const float d = (float)(t / (double)(rows * C));
    out3[0] = d;
    out3[1] = 0.f;
    out3[2] = d;
}

constexpr int DECODE_THREADS = 256, DECODE_WAVES = DECODE_THREADS / 64;

using seld_rows::DcaseRow;

// PER_CLASS: the threshold of a cell's three tracks is thresholds[class] (salsa_nn_seld_decode_multi_thr); otherwise the scalar
template <bool PER_CLASS>
__global__ __launch_bounds__(DECODE_THREADS) void seld_decode_multi_kernel(const float *__restrict__ act, const float *__restrict__ xyz,
                                                                           int n_in_frames, int n_frames, int C, float sed_threshold,
                                                                           const float *__restrict__ thresholds, double cos_unify,
                                                                           DcaseRow *__restrict__ rows, int *__restrict__ counts)
{
    __shared__ int wave_count[DECODE_WAVES];
    const size_t file = blockIdx.x;
    const int n_cells = n_frames * C, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float *fact = act + file * (size_t)n_in_frames * 3 * C;
    const float *fxyz = xyz + file * (size_t)n_in_frames * 9 * C;
    DcaseRow *frows = rows + file * (size_t)n_cells * 3;
    int base = 0;
    for (int tile = 0; tile < n_cells; tile += DECODE_THREADS) {            // (uniform trip count: every thread reaches the barriers)
        const int cell = tile + tid;
        const bool valid = cell < n_cells;
        const int frame = valid ? cell / C : 0, cls = valid ? cell - frame * C : 0;
        float out[9];
        int n_out = 0;
        if (valid) {
            float a[3], v[9];
            const float *pa = fact + (size_t)frame * 3 * C + cls, *pv = fxyz + (size_t)frame * 9 * C + cls;
#pragma unroll
            for (int n = 0; n < 3; n++) {
                a[n] = pa[n * C];
#pragma unroll
                for (int k = 0; k < 3; k++) v[n * 3 + k] = pv[(3 * k + n) * C];
            }
            n_out = multi_accdoa::unify_cell(a, v, PER_CLASS ? thresholds[cls] : sed_threshold, cos_unify, out, nullptr);
        }
        const unsigned long long bit0 = __ballot(n_out & 1), bit1 = __ballot(n_out & 2), lower = (1ull << lane) - 1ull;
        if (lane == 0) wave_count[wave] = __popcll(bit0) + 2 * __popcll(bit1);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < DECODE_WAVES; w++) {
            const int c = wave_count[w];
            if (w < wave) before += c;
            total += c;
        }
        before += __popcll(bit0 & lower) + 2 * __popcll(bit1 & lower);
#pragma unroll
        for (int g = 0; g < 3; g++) {                                        // before + g < 3 n_cells: three rows per cell at most
            if (g >= n_out) break;
            DcaseRow r;
            r.frame = (int16_t)frame;
            r.cls = (int16_t)cls;
            seld_decode::xyz_to_angles(out[g * 3], out[g * 3 + 1], out[g * 3 + 2], &r.azimuth, &r.elevation);
            frows[before + g] = r;
        }
        base += total;
        __syncthreads();                                                    // wave_count is rewritten by the next tile
    }
    if (tid == 0) counts[file] = base;
}

// both decode exports: the argument checks and the launch, with the scalar or the per-class thresholds [C] on the device
int launch_decode_multi(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames, int n_real_classes,
                        float sed_threshold, const float *d_thresholds, bool per_class, double cos_unify, int16_t *rows, int *counts,
                        void *hip_stream)
{
    if (!act || !xyz || !rows || !counts || ((uintptr_t)rows & 7)) return -1;
    if (per_class && (!d_thresholds || ((uintptr_t)d_thresholds & 3))) return -1;
    if (n_files < 1 || n_frames < 1 || n_frames > 32767 || n_in_frames < n_frames || n_real_classes < 1 || n_real_classes > 32767) return -1;
    if ((int64_t)n_in_frames * 9 * n_real_classes > INT32_MAX / 4) return -1;  // cell indices and 9 C columns stay in int
    if (!(cos_unify >= -1.0 && cos_unify <= 1.0)) return -1;                   // (NaN fails both comparisons)
    if (per_class)
        hipLaunchKernelGGL(seld_decode_multi_kernel<true>, dim3((unsigned)n_files), dim3(DECODE_THREADS), 0, (hipStream_t)hip_stream, act, xyz,
                           n_in_frames, n_frames, n_real_classes, 0.0f, d_thresholds, cos_unify, (DcaseRow *)rows, counts);
    else
        hipLaunchKernelGGL(seld_decode_multi_kernel<false>, dim3((unsigned)n_files), dim3(DECODE_THREADS), 0, (hipStream_t)hip_stream, act, xyz,
                           n_in_frames, n_frames, n_real_classes, sed_threshold, (const float *)nullptr, cos_unify, (DcaseRow *)rows, counts);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // namespace

extern "C" int salsa_nn_adpit_loss(const float *doa, const float *sed_gt, const float *doa_gt, int64_t rows, int n_real_classes,
                                   float *out3, float *g_logit, float *g_doa, uint8_t *chosen, double *partial_ws, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!doa || !sed_gt || !doa_gt || !out3 || !g_doa || !partial_ws) return -1;
    if (rows < 1 || n_real_classes < 1 || n_real_classes > 1024) return -1;
    if (rows >= INT32_MAX || rows * 9 * (int64_t)n_real_classes >= INT32_MAX) return -1;
    hipLaunchKernelGGL(adpit_loss_partial_kernel, dim3(ADPIT_BLOCKS), dim3(ADPIT_THREADS), 0, (hipStream_t)hip_stream, doa, sed_gt,
                       doa_gt, (long)rows, n_real_classes, g_logit, g_doa, chosen, partial_ws);
    hipLaunchKernelGGL(adpit_loss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, (const double *)partial_ws, (long)rows,
                       n_real_classes, out3);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_seld_decode_multi(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames,
                                          int n_real_classes, float sed_threshold, double cos_unify, int16_t *rows, int *counts,
                                          void *hip_stream)
{
    return launch_decode_multi(act, xyz, n_files, n_in_frames, n_frames, n_real_classes, sed_threshold, nullptr, false, cos_unify, rows, counts,
                               hip_stream);
}

extern "C" int salsa_nn_seld_decode_multi_thr(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames,
                                              int n_real_classes, const float *d_thresholds, double cos_unify, int16_t *rows, int *counts,
                                              void *hip_stream)
{
    return launch_decode_multi(act, xyz, n_files, n_in_frames, n_frames, n_real_classes, 0.0f, d_thresholds, true, cos_unify, rows, counts,
                               hip_stream);
}
