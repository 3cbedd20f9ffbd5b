// feature_utils.hip -- the entry points of include/salsa_hip.h that take no plan, each a small gfx950 kernel with its argument checks:
// salsa_scaler_accumulate, salsa_normalize_batch, salsa_to_freq_major, salsa_resample_batch, salsa_pcm_to_planar, salsa_augment_batch,
// salsa_augment_gcc_batch (per-element body: bank_batch.h) and salsa_selftest_decibel (K1's db10 on its own).
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include "salsa_internal.h"
#include <type_traits>
#include "bank_batch.h"

using namespace salsa_impl;

namespace {

// ------------------------------------------------------------------------------------------------------------ scaler
// compute_scaler (:204-262) on device: float64 sum and sum of squares over time of the first n_sc channels, per
// frequency.  One block per (clip, channel, tile of 64 frames); lane = frequency (coalesced rows; frequencies beyond 256 in further
// trips); one float64 atomic pair per frequency per block.  sums: [2][n_sc][F] (sum, sumsq), accumulated into (caller zeroes it once).
__global__ __launch_bounds__(256) void scaler_accumulate_kernel(const float *__restrict__ feat, int C, int T, int F,
                                                                int n_sc, double *__restrict__ sums)
{
    const int c = blockIdx.y, b = blockIdx.z;
    const int t0 = blockIdx.x * 64, t1 = t0 + 64 < T ? t0 + 64 : T;
    for (int f = threadIdx.x; f < F; f += 256) { // (one trip while F <= 256; SALSA-Lite at n_fft 1024 has F = 382)
        const float *p = feat + (((long)b * C + c) * T) * F + f;
        double s = 0.0, ss = 0.0;
        for (int t = t0; t < t1; t++) {
            const double v = (double)p[(long)t * F];
            s += v;
            ss += v * v;
        }
        atomicAdd(&sums[(long)c * F + f], s);
        atomicAdd(&sums[((long)n_sc + c) * F + f], ss);
    }
}

// normalise-on-load (dataset/database.py:197-202): feature[:n_sc] = (feature[:n_sc] - mean) / std, in place;
// mean/std: [n_sc][F] float32.  Channels >= n_sc (the spatial channels) are left untouched.
__global__ __launch_bounds__(256) void normalize_kernel(float *__restrict__ feat, long rows, int C, int T, int F, int n_sc,
                                                        const float *__restrict__ mean, const float *__restrict__ std)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); // one wave per (b, c, t) row of F floats
    if (row >= rows) return;
    const int t = (int)(row % T);
    const int c = (int)((row / T) % n_sc);
    const long b = row / ((long)T * n_sc);
    float *p = feat + ((b * C + c) * T + t) * F;
    for (int f = threadIdx.x & 63; f < F; f += 64) p[f] = (p[f] - mean[c * F + f]) / std[c * F + f];
}

// [rows][T][F] float32 (time-major, what the extract kernels write) -> [rows][F][T] float64 (the freq-major float64
// array contrib/salsa_flexible.py returns, :264).  64 x 64 tiles through LDS (+1 padding), both sides coalesced.
__global__ __launch_bounds__(256) void to_freq_major_kernel(const float *__restrict__ in, double *__restrict__ out, int T, int F)
{
    __shared__ float tile[64][65];
    const long row = blockIdx.z;
    const int t0 = blockIdx.y * 64, f0 = blockIdx.x * 64;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const float *src = in + row * (long)T * F;
    double *dst = out + row * (long)T * F;
    for (int i = ly; i < 64; i += 4)
        if (t0 + i < T && f0 + lx < F) tile[i][lx] = src[(long)(t0 + i) * F + f0 + lx];
    __syncthreads();
    for (int i = ly; i < 64; i += 4)
        if (f0 + i < F && t0 + lx < T) dst[(long)(f0 + i) * T + t0 + lx] = (double)tile[lx][i];
}

// ------------------------------------------------------------------------------------------------------------- resampling
// The resampling step of the reference's loader: librosa.load(path, sr=fs) (salsa_feature_extraction.py:353, lite :93) on a
// file of another native rate calls librosa 0.8.0 core/audio.py::resample -> resampy 0.2.2 (requirements.yml:181)
// resample(x, sr_orig, sr_new, filter='kaiser_best'): a windowed-sinc interpolator whose inner loop (resampy/interpn.py
// ::resample_f, numba) walks the filter's left wing from sample n = int(time_register) downwards and its right wing from
// n + 1 upwards, with the filter linearly interpolated between table entries and the float32 output element updated in
// place -- i.e. every tap is `y = float32(float64(y) + weight * float64(x))`, left wing first.  One thread per output
// sample does exactly that sequence (no FMA contraction), so the result is the sequential loop's bit for bit.  The
// filter table, its first differences and the time registers (a sequential float64 accumulation in the reference) are
// the caller's: salsa_amd/resample.py builds them once per (rate pair, length).  Bandwidth is irrelevant here (n_out x
// ~2 * 64 / scale taps from L2-resident tables): it is a loader step, not the hot path.
__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ x, float *__restrict__ y, long n_in, long n_out,
                                                       long n_fix, const double *__restrict__ win, const double *__restrict__ delta,
                                                       int nwin, int num_table, double scale, int index_step,
                                                       const double *__restrict__ treg)
{
#pragma clang fp contract(off)
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= n_fix) return;
    const long row = blockIdx.y;
    const float *xr = x + row * n_in;
    float acc = 0.f;                                     // (t >= n_out: librosa's fix_length pads with zeros)
    if (t < n_out) {
        const double tr = treg[t];
        const long n = (long)tr;
        double frac = scale * (tr - (double)n);
        double index_frac = frac * (double)num_table;
        int offset = (int)index_frac;
        double eta = index_frac - (double)offset;
        long m = (nwin - offset) / index_step;
        const long i_max = n + 1 < m ? n + 1 : m;
        for (long i = 0; i < i_max; i++) {
            const long idx = offset + i * index_step;
            const double w = win[idx] + eta * delta[idx];
            acc = (float)((double)acc + w * (double)xr[n - i]);
        }
        frac = scale - frac;
        index_frac = frac * (double)num_table;
        offset = (int)index_frac;
        eta = index_frac - (double)offset;
        m = (nwin - offset) / index_step;
        const long k_max = n_in - n - 1 < m ? n_in - n - 1 : m;
        for (long k = 0; k < k_max; k++) {
            const long idx = offset + k * index_step;
            const double w = win[idx] + eta * delta[idx];
            acc = (float)((double)acc + w * (double)xr[n + k + 1]);
        }
    }
    y[row * n_fix + t] = acc;
}

// ---------------------------------------------------------------------------------------------------------- PCM -> planar float32
// What librosa.load(path, sr=fs, mono=False, dtype=np.float32) (salsa_feature_extraction.py:353) does to a WAV file's samples before
// anything else: soundfile reads the interleaved PCM frames as float32 (libsndfile's normalisation: int16 / 2^15, int32 / 2^31,
// uint8 (x - 128) / 2^7, float32 as is -- all exact in float32 up to the one rounding of a 32-bit integer) and librosa transposes to
// (channels, samples).  The file pipeline uploads the file's data chunk as it is (half the PCIe bytes for 16-bit clips, no host
// arithmetic) and this kernel converts + de-interleaves: one thread per frame, one vector load of the frame's samples, one
// coalesced 4-byte store per channel plane.
template <typename S, int NCH> __device__ __forceinline__ void pcm_frame(const void *pcm, long n, float *v)
{
    struct alignas(sizeof(S) * NCH) vec { S x[NCH]; };
    const vec f = ((const vec *)pcm)[n];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        if constexpr (sizeof(S) == 2) v[c] = (float)f.x[c] * (1.0f / 32768.0f);
        else if constexpr (sizeof(S) == 1) v[c] = ((float)f.x[c] - 128.0f) * (1.0f / 128.0f);
        else if constexpr (std::is_same<S, int>::value) v[c] = (float)((double)f.x[c] * (1.0 / 2147483648.0));
        else v[c] = f.x[c];
    }
}
template <typename S> __global__ __launch_bounds__(256) void pcm_to_planar_kernel(const void *__restrict__ pcm, float *__restrict__ out, long n_frames, int nch)
{
    const long n = blockIdx.x * 256L + threadIdx.x;
    if (n >= n_frames) return;
    if (nch == 4) {
        float v[4];
        pcm_frame<S, 4>(pcm, n, v);
#pragma unroll
        for (int c = 0; c < 4; c++) out[c * n_frames + n] = v[c];
    } else {
        for (int c = 0; c < nch; c++) {
            float v[1];
            pcm_frame<S, 1>(pcm, n * nch + c, v);
            out[c * n_frames + n] = v[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ augmentation
// The reference's SALSA training augmentation (utilities/transforms.py; recipe in dataset/datamodule.py:45-52, :73-82) as
// ONE gather pass over a feature batch [B][7][T][F]: channel swap (FOA :394-437 / MIC :469-523, applied in the reference's
// order with its float32 arithmetic: the MIC swap re-references the three phase rows by differences), frequency shift with
// reflect padding (:298-320), then the cutout rectangles (:87-121, :149-194, :223-254; last rectangle wins; the spatial rows
// get zeros).  One thread = all 7 channels of one (clip, frame, bin).  par: int32 [B][AUG_NPAR] = m0..m3, shift, up, 0, 0,
// top[8], h[8], left[8], w[8] ; uval: float32 [B][8] in [0,1) ; minmax: float32 [B][2] -> fill = min + (max - min) * u.
constexpr int AUG_NPAR = bank_batch::NPAR;
// (the per-element body is bank_batch.h's, shared with salsa_bank_batch)
__global__ __launch_bounds__(256) void augment_kernel(const float *__restrict__ in, long in_batch, long in_chan,
                                                      float *__restrict__ out, int T, int F,
                                                      int format, int n_zero, const int *__restrict__ par,
                                                      const float *__restrict__ uval, const float *__restrict__ minmax)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * F) return;
    const int t = i / F, f = i - t * F;
    const long plane = (long)T * F;
    // the input may be a time-cropped view: its own batch / channel strides
    bank_batch::augment7(in + (long)b * in_batch, in_chan, out + (long)b * 7 * plane + i, plane, t, f, F, format != SALSA_FORMAT_FOA,
                         n_zero, par + b * AUG_NPAR, uval + b * 8, minmax + 2 * b);
}

// The baseline GCC recipe (dataset/datamodule.py:83-100) on [B][10][T][F] = M1..M4 | xc12 xc13 xc14 xc23 xc24 xc34: the
// GccRandomSwapChannelMic permutation (transforms.py:568-602; its branches are if / elif / elif, so only the FIRST set bit of
// m0..m2 acts on the features), some GCC rows also flipped along the lag axis (f -> F-1-f); RandomShiftUpDownNp with
// n_last_channels = 6 (only the four spectrogram rows shift); the cutout rectangles with the last 6 rows zeroed.  Pure gathers:
// every output value is an input value or the fill value.  One thread = all 10 channels of one (clip, frame, bin).
__global__ __launch_bounds__(256) void augment_gcc_kernel(const float *__restrict__ in, long in_batch, long in_chan,
                                                          float *__restrict__ out, int T, int F, const int *__restrict__ par,
                                                          const float *__restrict__ uval, const float *__restrict__ minmax)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * F) return;
    const int t = i / F, f = i - t * F;
    const long plane = (long)T * F;
    bank_batch::augment10(in + (long)b * in_batch, in_chan, out + (long)b * 10 * plane + i, plane, t, f, F, par + b * AUG_NPAR,
                          uval + b * 8, minmax + 2 * b);
}

__global__ __launch_bounds__(256) void db10_kernel(const float *__restrict__ p, float *__restrict__ o, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) o[i] = db10(p[i]);
}

} // namespace

extern "C" {

int salsa_scaler_accumulate(const float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq,
                            int n_scaler_channels, double *d_sums, void *hip_stream)
{
    if (!d_feat || !d_sums || batch <= 0 || n_channels <= 0 || n_frames <= 0 || n_freq <= 0 ||
        n_scaler_channels <= 0 || n_scaler_channels > n_channels || n_frames >= INT32_MAX)
        return fail(SALSA_EINVAL, "salsa_scaler_accumulate: bad argument%s");
    if (batch > 65535 || n_scaler_channels > 65535) // grid z and grid y
        return fail(SALSA_EINVAL, "salsa_scaler_accumulate: batch or scaler channels exceed one launch's grid%s");
    dim3 grid((unsigned)((n_frames + 63) / 64), (unsigned)n_scaler_channels, (unsigned)batch);
    hipLaunchKernelGGL(scaler_accumulate_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, d_feat, n_channels,
                       (int)n_frames, n_freq, n_scaler_channels, d_sums);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_normalize_batch(float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq, int n_scaler_channels,
                          const float *d_mean, const float *d_std, void *hip_stream)
{
    if (!d_feat || !d_mean || !d_std || batch <= 0 || n_channels <= 0 || n_frames <= 0 || n_freq <= 0 ||
        n_scaler_channels <= 0 || n_scaler_channels > n_channels || n_frames >= INT32_MAX)
        return fail(SALSA_EINVAL, "salsa_normalize_batch: bad argument%s");
    const long rows = (long)batch * n_scaler_channels * n_frames;
    if ((rows + 3) / 4 >= INT32_MAX) return fail(SALSA_EINVAL, "salsa_normalize_batch: too many rows for one launch%s");
    hipLaunchKernelGGL(normalize_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)hip_stream, d_feat,
                       rows, n_channels, (int)n_frames, n_freq, n_scaler_channels, d_mean, d_std);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_augment_batch(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch,
                        int64_t n_frames, int n_freq, int audio_format, int n_zero_channels, const int *d_params,
                        const float *d_uval, const float *d_minmax, void *hip_stream)
{
    if (in_channel_stride < n_frames * n_freq || in_batch_stride < 7 * in_channel_stride)
        return fail(SALSA_EINVAL, "salsa_augment_batch: input strides smaller than the [7][T][F] block%s");
    if (!d_in || !d_out || d_in == d_out || !d_params || !d_uval || !d_minmax || batch <= 0 || batch > 65535 || n_frames <= 0 ||
        n_freq <= 1 || n_frames * n_freq >= INT32_MAX || n_zero_channels < 0 || n_zero_channels > 7)
        return fail(SALSA_EINVAL, "salsa_augment_batch: bad argument%s");
    if (audio_format != SALSA_FORMAT_FOA && audio_format != SALSA_FORMAT_MIC) return fail(SALSA_EFORMAT, "Unknown audio format%s");
    const long n = (long)n_frames * n_freq;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)hip_stream,
                       d_in, (long)in_batch_stride, (long)in_channel_stride, d_out, (int)n_frames, n_freq, audio_format,
                       n_zero_channels, d_params, d_uval, d_minmax);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_augment_gcc_batch(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch,
                            int64_t n_frames, int n_freq, const int *d_params, const float *d_uval, const float *d_minmax,
                            void *hip_stream)
{
    if (in_channel_stride < n_frames * n_freq || in_batch_stride < 10 * in_channel_stride)
        return fail(SALSA_EINVAL, "salsa_augment_gcc_batch: input strides smaller than the [10][T][F] block%s");
    if (!d_in || !d_out || d_in == d_out || !d_params || !d_uval || !d_minmax || batch <= 0 || batch > 65535 || n_frames <= 0 ||
        n_freq <= 1 || n_frames * n_freq >= INT32_MAX)
        return fail(SALSA_EINVAL, "salsa_augment_gcc_batch: bad argument%s");
    const long n = (long)n_frames * n_freq;
    hipLaunchKernelGGL(augment_gcc_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, (hipStream_t)hip_stream,
                       d_in, (long)in_batch_stride, (long)in_channel_stride, d_out, (int)n_frames, n_freq, d_params, d_uval, d_minmax);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_selftest_decibel(const float *d_power, float *d_db, int64_t n, void *hip_stream)
{
    if (!d_power || !d_db || n <= 0 || (n + 255) / 256 >= INT32_MAX) return fail(SALSA_EINVAL, "salsa_selftest_decibel: bad argument%s");
    hipLaunchKernelGGL(db10_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, d_power, d_db, (long)n);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_to_freq_major(const float *d_feat, int64_t n_rows, int64_t n_frames, int n_freq, double *d_out, void *hip_stream)
{
    if (!d_feat || !d_out || n_rows <= 0 || n_frames <= 0 || n_freq <= 0 || n_rows > 65535 || (n_frames + 63) / 64 > 65535)
        return fail(SALSA_EINVAL, "salsa_to_freq_major: bad argument%s");
    dim3 grid((unsigned)((n_freq + 63) / 64), (unsigned)((n_frames + 63) / 64), (unsigned)n_rows);
    hipLaunchKernelGGL(to_freq_major_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, d_feat, d_out, (int)n_frames, n_freq);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_resample_batch(const float *d_x, int n_rows, int64_t n_in, float *d_y, int64_t n_out, int64_t n_out_fixed, double sample_ratio,
                         const double *d_interp_win, const double *d_interp_delta, int n_win, int num_table,
                         const double *d_time_register, void *hip_stream)
{
    if (!d_x || !d_y || !d_interp_win || !d_interp_delta || !d_time_register || n_rows <= 0 || n_rows > 65535 || n_in <= 0 ||
        n_out < 0 || n_out_fixed < n_out || n_out_fixed <= 0 || !(sample_ratio > 0.0) || n_win <= 0 || num_table <= 0 ||
        (n_out_fixed + 255) / 256 >= INT32_MAX)
        return fail(SALSA_EINVAL, "salsa_resample_batch: bad argument%s");
    const double scale = sample_ratio < 1.0 ? sample_ratio : 1.0;          // resampy/interpn.py: scale = min(1.0, sample_ratio)
    const int index_step = (int)(scale * (double)num_table);              //                     index_step = int(scale * num_table)
    if (index_step < 1) return fail(SALSA_EINVAL, "salsa_resample_batch: sample_ratio * num_table < 1%s");
    dim3 grid((unsigned)((n_out_fixed + 255) / 256), (unsigned)n_rows);
    hipLaunchKernelGGL(resample_kernel, grid, dim3(256), 0, (hipStream_t)hip_stream, d_x, d_y, (long)n_in, (long)n_out, (long)n_out_fixed,
                       d_interp_win, d_interp_delta, n_win, num_table, scale, index_step, d_time_register);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

int salsa_pcm_to_planar(const void *d_pcm, int sample_format, int n_channels, int64_t n_frames, float *d_out, void *hip_stream)
{
    if (!d_pcm || !d_out || n_channels <= 0 || n_channels > 64 || n_frames <= 0 || (n_frames + 255) / 256 >= INT32_MAX)
        return fail(SALSA_EINVAL, "salsa_pcm_to_planar: bad argument%s");
    const size_t fb = (size_t)n_channels * (sample_format == SALSA_PCM_S16 ? 2 : sample_format == SALSA_PCM_U8 ? 1 : 4);
    if (n_channels == 4 && ((uintptr_t)d_pcm % fb)) return fail(SALSA_EINVAL, "salsa_pcm_to_planar: d_pcm must be aligned to one frame%s");
    dim3 grid((unsigned)((n_frames + 255) / 256));
    hipStream_t s = (hipStream_t)hip_stream;
    switch (sample_format) {
    case SALSA_PCM_S16: hipLaunchKernelGGL(pcm_to_planar_kernel<short>, grid, dim3(256), 0, s, d_pcm, d_out, (long)n_frames, n_channels); break;
    case SALSA_PCM_S32: hipLaunchKernelGGL(pcm_to_planar_kernel<int>, grid, dim3(256), 0, s, d_pcm, d_out, (long)n_frames, n_channels); break;
    case SALSA_PCM_U8: hipLaunchKernelGGL(pcm_to_planar_kernel<unsigned char>, grid, dim3(256), 0, s, d_pcm, d_out, (long)n_frames, n_channels); break;
    case SALSA_PCM_F32: hipLaunchKernelGGL(pcm_to_planar_kernel<float>, grid, dim3(256), 0, s, d_pcm, d_out, (long)n_frames, n_channels); break;
    default: return fail(SALSA_EINVAL, "salsa_pcm_to_planar: unknown sample format%s");
    }
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

} // extern "C"
