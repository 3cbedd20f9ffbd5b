// seld_decode.hip -- salsa_nn_seld_decode (include/salsa_nn.h): the last stage of inference on the device.  The label-rate chunk
// outputs of a batch of files are combined into file predictions (reference models/interfaces.py:97-139, combine_chunks), the SED
// threshold is applied and the active (frame, class) pairs are written as DCASE rows (frame, class, azimuth, elevation) in the
// reference's order (:232-256): a few hundred 8-byte rows per file leave the device instead of the 600 x 48 floats.
//
// One workgroup of 256 threads (4 waves) per file.  The file's n_frames * nc pairs are walked in tiles of 256 CONSECUTIVE pairs
// (pair = frame * nc + class, i.e. np.nonzero's order); a tile is compacted with one ballot per wave (the lane's rank is the popcount
// of the lower lanes' bits), the four wave counts go through LDS, and a running base carries the rows written by earlier tiles, so
// the rows come out sorted with no atomics and the result does not depend on timing.  The arithmetic is seld_decode.h's.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "seld_decode.h"
#include "seld_rows.h" // DcaseRow

namespace {

constexpr int DECODE_THREADS = 256, DECODE_WAVES = DECODE_THREADS / 64;

using seld_rows::DcaseRow;

// PER_CLASS: the threshold of a pair is thresholds[class] (salsa_nn_seld_decode_thr); otherwise the scalar, and thresholds is not read
template <bool PER_CLASS>
__global__ __launch_bounds__(DECODE_THREADS) void seld_decode_kernel(const float *__restrict__ sed, const float *__restrict__ xyz,
                                                                     int n_chunks, int chunk_len, int chunk_hop, int n_frames, int nc,
                                                                     float sed_threshold, const float *__restrict__ thresholds, int gmean,
                                                                     DcaseRow *__restrict__ rows, int *__restrict__ counts,
                                                                     float *__restrict__ file_sed, float *__restrict__ file_xyz)
{
    __shared__ int wave_count[DECODE_WAVES];
    const size_t file = blockIdx.x;
    const int n_pairs = n_frames * nc, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float *fsed = sed + file * (size_t)n_chunks * chunk_len * nc;
    const float *fxyz = xyz + file * (size_t)n_chunks * chunk_len * 3 * nc;
    DcaseRow *frows = rows + file * (size_t)n_pairs;
    int base = 0;
    for (int tile = 0; tile < n_pairs; tile += DECODE_THREADS) {          // (uniform trip count: every thread reaches the barriers)
        const int pair = tile + tid;
        const bool valid = pair < n_pairs;
        const int frame = valid ? pair / nc : 0, cls = valid ? pair - frame * nc : 0;
        bool active = false;
        if (valid) {
            const float s = seld_decode::file_value(fsed, n_chunks, chunk_len, chunk_hop, n_frames, nc, frame, cls, gmean);
            if (file_sed) file_sed[file * (size_t)n_pairs + pair] = s;
            active = seld_decode::is_active(s, PER_CLASS ? thresholds[cls] : sed_threshold);
        }
        const unsigned long long mask = __ballot(active);
        if (lane == 0) wave_count[wave] = __popcll(mask);
        __syncthreads();
        int before = base, total = 0;
        for (int w = 0; w < DECODE_WAVES; w++) {
            const int c = wave_count[w];
            if (w < wave) before += c;
            total += c;
        }
        if (valid && (active || file_xyz)) {
            float v[3];
            for (int k = 0; k < 3; k++) {
                v[k] = seld_decode::file_value(fxyz, n_chunks, chunk_len, chunk_hop, n_frames, 3 * nc, frame, k * nc + cls, gmean);
                if (file_xyz) file_xyz[(file * (size_t)n_frames + frame) * 3 * nc + k * nc + cls] = v[k];
            }
            if (active) {
                DcaseRow r;
                r.frame = (int16_t)frame;
                r.cls = (int16_t)cls;
                seld_decode::xyz_to_angles(v[0], v[1], v[2], &r.azimuth, &r.elevation);
                frows[before + __popcll(mask & ((1ull << lane) - 1ull))] = r;   // < n_pairs: one row per active pair at most
            }
        }
        base += total;
        __syncthreads();                                                    // wave_count is rewritten by the next tile
    }
    if (tid == 0) counts[file] = base;
}

// both exports: the argument checks and the launch, with the scalar or the per-class thresholds [nc] on the device
int launch_decode(const float *sed, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop, int n_frames, int nc,
                  float sed_threshold, const float *d_thresholds, bool per_class, int combine, int16_t *rows, int *counts, float *file_sed,
                  float *file_xyz, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!sed || !xyz || !rows || !counts || ((uintptr_t)rows & 7)) return -1;
    if (per_class && (!d_thresholds || ((uintptr_t)d_thresholds & 3))) return -1;
    if (n_files < 1 || n_chunks < 1 || n_frames < 1 || n_frames > 32767 || nc < 1 || nc > 32767 || chunk_hop < 1 || chunk_len < 1) return -1;
    if ((int64_t)n_frames * nc > INT32_MAX / 4) return -1;                  // pair indices and 3 nc columns stay in int
    if (combine != 0 && combine != 1) return -1;
    if (n_chunks > 1 && (chunk_hop > chunk_len || chunk_len > n_frames)) return -1;
    if (n_chunks != seld_decode::expected_chunks(n_frames, chunk_len, chunk_hop)) return -1;
    if (per_class)
        hipLaunchKernelGGL(seld_decode_kernel<true>, dim3((unsigned)n_files), dim3(DECODE_THREADS), 0, (hipStream_t)hip_stream, sed, xyz,
                           n_chunks, chunk_len, chunk_hop, n_frames, nc, 0.0f, d_thresholds, combine, (DcaseRow *)rows, counts, file_sed, file_xyz);
    else
        hipLaunchKernelGGL(seld_decode_kernel<false>, dim3((unsigned)n_files), dim3(DECODE_THREADS), 0, (hipStream_t)hip_stream, sed, xyz,
                           n_chunks, chunk_len, chunk_hop, n_frames, nc, sed_threshold, (const float *)nullptr, combine, (DcaseRow *)rows, counts,
                           file_sed, file_xyz);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // namespace

extern "C" int salsa_nn_seld_decode(const float *sed, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop,
                                    int n_frames, int nc, float sed_threshold, int combine, int16_t *rows, int *counts, float *file_sed,
                                    float *file_xyz, void *hip_stream)
{
    return launch_decode(sed, xyz, n_files, n_chunks, chunk_len, chunk_hop, n_frames, nc, sed_threshold, nullptr, false, combine, rows, counts,
                         file_sed, file_xyz, hip_stream);
}

extern "C" int salsa_nn_seld_decode_thr(const float *sed, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop,
                                        int n_frames, int nc, const float *d_thresholds, int combine, int16_t *rows, int *counts,
                                        float *file_sed, float *file_xyz, void *hip_stream)
{
    return launch_decode(sed, xyz, n_files, n_chunks, chunk_len, chunk_hop, n_frames, nc, 0.0f, d_thresholds, true, combine, rows, counts,
                         file_sed, file_xyz, hip_stream);
}
