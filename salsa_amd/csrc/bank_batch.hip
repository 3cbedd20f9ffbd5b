// bank_batch.hip -- salsa_bank_batch (include/salsa_hip.h): one training batch straight from the feature bank.  The bank holds every
// clip's features back to back, float32 [C][bank_frames][F] (the reference's concatenated layout, dataset/database.py:230-231), and a
// training chunk is a window of chunk_frames frames of it; the composed path slices B windows, stacks them, augments the stack and
// swaps the targets -- about a hundred small launches.  Here the gather IS the augmentation's load: the per-element body of
// salsa_augment_batch (bank_batch.h) reads channel c of sample b at bank + (c * bank_frames + start[b]) * F instead of a stacked copy,
// so the result equals the composed one bit for bit and the stacked copy is never written.
//
// Launches, all on the caller's stream, no host synchronisation:
//   1. bank_labels_kernel   sed / doa windows of the label banks, the target half of the swap applied; its first thread per sample
//                           also resets the sample's min / max keys
//   2. bank_minmax_kernel   ONLY when the host drew a rectangle: min / max of every unaugmented chunk (the cutout's fill range) into
//                           [B][2] order-preserving integer keys with one atomic pair per block -- min and max do not depend on the
//                           order, so the result does not depend on timing
//   3. bank_gather_kernel   one thread = all C channels of one (sample, frame, bin): pure streaming, dword loads coalesced along the
//                           frequency rows (F may be odd: rows are not 16-byte aligned, so no wider loads)
// Every bank offset is 64-bit: the real bank [7][1 920 000][200] has 2.69e9 elements.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "bank_batch.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int MM_THREADS = 256, MM_PER_THREAD = 16, MM_TILE = MM_THREADS * MM_PER_THREAD;

// float -> unsigned key with the same order (negative floats: all bits flipped; others: the sign bit set)
__device__ __forceinline__ unsigned order_key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// a start the bank does not hold (the Python layer refuses it before the call): such a sample is left unwritten, never read
__device__ __forceinline__ bool window_ok(int64_t s, int64_t len, int64_t total) { return s >= 0 && s <= total - len; }

__global__ __launch_bounds__(256) void bank_labels_kernel(const float *__restrict__ sed_all, const float *__restrict__ doa_all,
                                                          int64_t label_total, int nc, const int64_t *__restrict__ gt_start, int L,
                                                          int recipe, const int *__restrict__ par, float *__restrict__ sed,
                                                          float *__restrict__ doa, unsigned *__restrict__ mm_keys)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && mm_keys) { mm_keys[2 * b] = 0xffffffffu; mm_keys[2 * b + 1] = 0u; }
    const int64_t g = gt_start[b];
    if (!window_ok(g, L, label_total)) return;
    const int n_sed = L * nc;
    if (i < n_sed) {
        sed[(int64_t)b * n_sed + i] = sed_all[g * nc + i];                 // a window of label frames is contiguous
    } else if (i < 4 * n_sed) {
        const int j = i - n_sed, l = j / (3 * nc), col = j - l * 3 * nc;
        const float *row = doa_all + (g + l) * 3 * nc;
        doa[(int64_t)b * 3 * n_sed + j] = recipe == bank_batch::RECIPE_NONE
                                              ? row[col]
                                              : bank_batch::swap_target(row, col, nc, recipe == bank_batch::RECIPE_FOA, par + b * bank_batch::NPAR);
    }
}

// grid (tiles of one channel's window, C, B): channel c of sample b is ONE contiguous run of T * F floats of the bank
__global__ __launch_bounds__(MM_THREADS) void bank_minmax_kernel(const float *__restrict__ bank, int64_t bank_frames, int F,
                                                                 const int64_t *__restrict__ start, int T, unsigned *__restrict__ mm_keys)
{
    __shared__ float s_lo[MM_THREADS / 64], s_hi[MM_THREADS / 64];
    const int b = blockIdx.z, c = blockIdx.y, tid = threadIdx.x;
    const int64_t s = start[b];
    if (!window_ok(s, T, bank_frames)) return;                            // (uniform over the block)
    const float *run = bank + ((int64_t)c * bank_frames + s) * F;
    const int n = T * F;
    float lo = __int_as_float(0x7f800000), hi = -lo;
    const int base = blockIdx.x * MM_TILE + tid;
#pragma unroll
    for (int k = 0; k < MM_PER_THREAD; k++) {
        const int i = base + k * MM_THREADS;
        if (i < n) {
            const float v = run[i];
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off));
        hi = fmaxf(hi, __shfl_xor(hi, off));
    }
    if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MM_THREADS / 64; w++) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
        atomicMin(&mm_keys[2 * b], order_key(lo));
        atomicMax(&mm_keys[2 * b + 1], order_key(hi));
    }
}

__global__ __launch_bounds__(256) void bank_gather_kernel(const float *__restrict__ bank, int C, int64_t bank_frames, int F,
                                                          const int64_t *__restrict__ start, int T, int recipe, int n_zero,
                                                          const int *__restrict__ par, const float *__restrict__ uval,
                                                          const unsigned *__restrict__ mm_keys, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * F) return;
    const int64_t s = start[b];
    if (!window_ok(s, T, bank_frames)) return;
    const int t = i / F, f = i - t * F;
    const int64_t plane = (int64_t)T * F, chan = bank_frames * F;
    const float *src = bank + s * F;                                       // (channel 0, frame 0) of the sample
    float *dst = out + (int64_t)b * C * plane + i;
    if (recipe == bank_batch::RECIPE_NONE) {
        for (int c = 0; c < C; c++) dst[c * plane] = src[c * chan + i];
        return;
    }
    float mm[2] = {0.f, 0.f};                                              // no rectangle in the batch: never read
    if (mm_keys) { mm[0] = key_value(mm_keys[2 * b]); mm[1] = key_value(mm_keys[2 * b + 1]); }
    const int *p = par + b * bank_batch::NPAR;
    if (recipe == bank_batch::RECIPE_GCC)
        bank_batch::augment10(src, chan, dst, plane, t, f, F, p, uval + b * 8, mm);
    else
        bank_batch::augment7(src, chan, dst, plane, t, f, F, recipe == bank_batch::RECIPE_MIC, n_zero, p, uval + b * 8, mm);
}

int bfail(int code, const char *msg)
{
    salsa_set_last_error_(msg);
    return code;
}

} // namespace

extern "C" int salsa_bank_batch(const float *d_bank, int n_channels, int64_t bank_frames, int n_freq, const float *d_sed_all,
                                const float *d_doa_all, int64_t label_frames_total, int n_classes, const int64_t *d_start,
                                const int64_t *d_gt_start, int batch, int chunk_frames, int label_frames, int recipe,
                                int n_zero_channels, const int *d_params, const float *d_uval, int has_rects, float *d_x, float *d_sed,
                                float *d_doa, void *d_minmax_ws, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!d_bank || !d_start || !d_x || d_bank == d_x) return bfail(SALSA_EINVAL, "salsa_bank_batch: NULL bank, start or output");
    if (n_channels != 7 && n_channels != 10) return bfail(SALSA_EINVAL, "salsa_bank_batch: the bank has 7 or 10 channels");
    if (recipe < SALSA_BANK_NONE || recipe > SALSA_BANK_GCC) return bfail(SALSA_EINVAL, "salsa_bank_batch: unknown recipe");
    if ((recipe == SALSA_BANK_GCC) != (n_channels == 10) && recipe != SALSA_BANK_NONE)
        return bfail(SALSA_EINVAL, "salsa_bank_batch: the foa / mic recipes take 7 channels, the gcc recipe 10");
    if (batch <= 0 || batch > 65535 || n_freq <= 1 || chunk_frames <= 0 || bank_frames < chunk_frames ||
        (int64_t)chunk_frames * n_freq >= INT32_MAX || bank_frames > INT64_MAX / 16 / n_freq)
        return bfail(SALSA_EINVAL, "salsa_bank_batch: bad batch, frame or bin count");
    if (n_zero_channels < 0 || n_zero_channels > n_channels) return bfail(SALSA_EINVAL, "salsa_bank_batch: bad n_zero_channels");
    if (recipe != SALSA_BANK_NONE && (!d_params || !d_uval)) return bfail(SALSA_EINVAL, "salsa_bank_batch: a recipe needs d_params and d_uval");
    const bool labels = d_sed_all || d_doa_all || d_gt_start || d_sed || d_doa;
    if (labels) {
        if (!d_sed_all || !d_doa_all || !d_gt_start || !d_sed || !d_doa) return bfail(SALSA_EINVAL, "salsa_bank_batch: labels need both banks, gt_start and both outputs");
        if (n_classes < 1 || label_frames < 1 || label_frames_total < label_frames || (int64_t)label_frames * 4 * n_classes >= INT32_MAX ||
            label_frames_total > INT64_MAX / 16 / n_classes)
            return bfail(SALSA_EINVAL, "salsa_bank_batch: bad label frame or class count");
    }
    if (has_rects && (recipe == SALSA_BANK_NONE || !labels || !d_minmax_ws || ((uintptr_t)d_minmax_ws & 3)))
        return bfail(SALSA_EINVAL, "salsa_bank_batch: rectangles need a recipe, the label pass (it resets the workspace) and d_minmax_ws");
    hipStream_t st = (hipStream_t)hip_stream;
    unsigned *keys = has_rects ? (unsigned *)d_minmax_ws : nullptr;
    if (labels) {
        const int n = label_frames * 4 * n_classes;
        hipLaunchKernelGGL(bank_labels_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_sed_all, d_doa_all,
                           label_frames_total, n_classes, d_gt_start, label_frames, recipe, d_params, d_sed, d_doa, keys);
    }
    const int n = chunk_frames * n_freq;
    if (has_rects)
        hipLaunchKernelGGL(bank_minmax_kernel, dim3((unsigned)((n + MM_TILE - 1) / MM_TILE), (unsigned)n_channels, (unsigned)batch),
                           dim3(MM_THREADS), 0, st, d_bank, bank_frames, n_freq, d_start, chunk_frames, keys);
    hipLaunchKernelGGL(bank_gather_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, st, d_bank, n_channels,
                       bank_frames, n_freq, d_start, chunk_frames, recipe, n_zero_channels, d_params, d_uval, keys, d_x);
    if (hipGetLastError() != hipSuccess) return bfail(SALSA_EHIP, "salsa_bank_batch: launch failed");
    return SALSA_OK;
}
