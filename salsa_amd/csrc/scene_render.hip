// scene_render.hip -- labelled SELD scenes rendered on the device (include/salsa_hip.h: salsa_scene_*):
//   audio[b, c, n] = ambient[b, c, n] + sum_i g_i (h[r_i, c, :] * s_i)[n - o_i]        0 <= n < N, `*` the full linear convolution
// by uniformly partitioned overlap-save in float32.  A partition is 512 samples; the real 1024-point transform of two neighbouring
// partitions is a 512-point complex FFT, one wave with 8 points per lane (scene_fft.h has the per-lane arithmetic and the packed
// half-spectrum layout).  The clip has ONE block grid, output block m = samples [512 m, 512 (m + 1)); an item is laid onto that grid
// at its onset before it is transformed, so onsets need no alignment.
//
//   rir_spectra_kernel     once per bank: h[r, c, 512 p .. 512 p + 511] followed by 512 zeros -> H[r, c, p][k], behind the twiddle table
//   spectra_kernel         per item and input block j (samples [512 (j - 1), 512 (j + 1)) of the item on the clip's grid, only the
//                          blocks the dry event meets) -> X_i[j][k] in the caller's workspace
//   render_kernel          per (clip, output block m), one workgroup for all channels: Y_c[k] = sum_i sum_p g_i H[r_i, c, p][k]
//                          X_i[m - p][k] with items and partitions in ascending order, the inverse transform per channel, whose last 512
//                          samples are block m, then ambient + y where a sample lies in some item's support [o_i, o_i + len_i + L - 1)
//                          and the ambient's own bits (or zero) everywhere else, so that silence stays silent.
// Moving sources: the host has cut every item into segments, one per trajectory node; a segment is an item of
// its own response whose dry samples are weighted by a linear ramp while they are loaded, and a block table names the segments that
// reach each output block.  A static item is ONE segment of step 0, loaded as it is.  Both entry points run ONE body of each kernel,
// instantiated twice: spectra_kernel<RAMP> differs in the load of the dry samples (the window), render_kernel<BLOCKS> in the one
// statement that finds the rows [i_lo, i_hi) of a block (the clip's, or the block table's).  So a batch of static items goes through
// the same arithmetic in the same order by either entry.
// Nothing is summed across workgroups: no atomics, one fixed order, so two runs agree bit for bit and a clip does not depend on the
// rest of its batch.  All offsets are 64-bit.  The launchers check everything on the host before the first device call.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/salsa_hip.h"
#include "scene_fft.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

// the products of spec_mac are fmaf by hand; nothing else may be fused behind its back
#pragma clang fp contract(off)

namespace {

using scene::cf;
using scene::FFT_N;
using scene::Z_LEN;
using scene::zpad;

constexpr int SC_THREADS = 256, SC_WAVES = 4;
constexpr int SC_TW = 2 * FFT_N;            // twiddle table entries in front of the partition spectra
constexpr int SC_CH = 4;                    // channels accumulated in registers at a time by the render kernel: one wave each for the inverse
constexpr int SC_MAX_CH = 16, SC_MAX_RIR = 16384, SC_MAX_ITEMS = 256;   // limits of the launchers (include/salsa_hip.h)
constexpr int SC_MAX_SEGS = 65536;                  // segments per clip
constexpr int64_t SC_MIN_STEP = 240, SC_MAX_STEP = 1 << 24;   // ramp steps; up to 2^24 the window's numerator is exact in float32

// The 512-point forward transform of the eight points each lane of ONE wave holds (v[r] = z_in[lane + 64 r]) through that wave's
// LDS line; -> v[r] = Z[lane + 64 r].  Every wave of the workgroup calls it (the barriers are workgroup barriers), nobody may still be
// reading `z` at entry, and `z` is being read until the caller's next barrier.
__device__ inline void wave_fft(cf *v, cf *z, const cf *__restrict__ tw, int lane)
{
    salsa::dft8(v);
    scene::lane_store(v, z, lane, 1);
    __syncthreads();
    scene::lane_load(v, z, lane);
    scene::lane_pass(v, tw, lane, 8);
    __syncthreads();
    scene::lane_store(v, z, lane, 8);
    __syncthreads();
    scene::lane_load(v, z, lane);
    scene::lane_pass(v, tw, lane, 64);
}

// v[r] = x[2 t] + i x[2 t + 1], t = lane + 64 r, of 1024 real samples -> the packed half spectrum, s[r] = S[lane + 64 r]
__device__ inline void wave_real_spectrum(cf *v, cf *z, const cf *__restrict__ tw, int lane)
{
    wave_fft(v, z, tw, lane);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) z[zpad(lane + 64 * r)] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int k = lane + 64 * r;
        v[r] = scene::real_unpack(z[zpad(k)], z[zpad((FFT_N - k) & (FFT_N - 1))], k, tw);
    }
}

__global__ __launch_bounds__(256) void twiddle_kernel(cf *__restrict__ tw)
{
    const int m = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (m >= SC_TW) return;
    double s, c;
    sincospi((double)m / (double)FFT_N, &s, &c);              // W^m = exp(-2 pi i m / 1024)
    tw[m] = {(float)c, (float)-s};
}

__global__ __launch_bounds__(SC_THREADS) void rir_spectra_kernel(const float *__restrict__ rirs, int64_t n_units, int L, int P,
                                                                  cf *__restrict__ spectra)
{
    __shared__ cf zs[SC_WAVES][Z_LEN];
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const cf *tw = spectra;
    const int64_t u = (int64_t)blockIdx.x * SC_WAVES + w;     // (r, c, p) flattened
    const bool on = u < n_units;
    const int64_t rc = on ? u / P : 0;
    const int p = on ? (int)(u - rc * P) : 0;
    const float *h = rirs + rc * L;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t n = (int64_t)FFT_N * p + 2 * (lane + 64 * r);
        const bool first = on && r < 4;                       // the second half of the 1024 samples is zero
        v[r] = {first && n < L ? h[n] : 0.f, first && n + 1 < L ? h[n + 1] : 0.f};
    }
    wave_real_spectrum(v, zs[w], tw, lane);
    if (!on) return;
    cf *dst = spectra + SC_TW + u * FFT_N;
#pragma unroll
    for (int r = 0; r < 8; r++) dst[lane + 64 * r] = v[r];
}

// The tables of either entry point, as the kernels read them.  A row is an item (salsa_scene_render) or a segment (_moving).
struct scene_tables {
    const int *ranges;          // (B + 1) clip_start: clip b owns rows [ranges[b], ranges[b + 1]); or the block table (B, M, 2): the first
                                // and one-past-last row that can reach output block m of clip b
    const int64_t *rows;        // (4, n): source offset in `events`, onset, length, rir; segments have two more: (6, n) with the ramp's
                                // centre counted from the segment's start, and the ramp step
    const float *gains;         // (n)
    int n;
};

// RAMP: the rows are segments, whose dry samples are weighted by their ramp while they are loaded (step 0: no window); without it
// neither centre nor step is read, and a sample is loaded as it is
template <bool RAMP>
__global__ __launch_bounds__(SC_THREADS) void spectra_kernel(const float *__restrict__ events, const scene_tables tb, int slots, int64_t M,
                                                              const cf *__restrict__ tw, cf *__restrict__ ws)
{
    __shared__ cf zs[SC_WAVES][Z_LEN];
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int64_t i = blockIdx.x, n = tb.n;
    const int64_t src = tb.rows[i], o = tb.rows[n + i], len = tb.rows[2 * n + i];
    const int64_t centre = RAMP ? tb.rows[4 * n + i] : 0, step = RAMP ? tb.rows[5 * n + i] : 0;
    const int64_t j0 = o >> 9, j1 = min(((o + len - 1) >> 9) + 1, M - 1);
    const int slot = (int)blockIdx.y * SC_WAVES + w;
    const int64_t j = j0 + slot;
    const bool on = slot < slots && j <= j1;
    const float fstep = (float)step;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t e = FFT_N * (j - 1) + 2 * (lane + 64 * r) - o;      // index into the row's dry samples
        float x[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int64_t eq = e + q;
            const bool in = on && eq >= 0 && eq < len;
            x[q] = in ? events[src + eq] : 0.f;
            if (in && step) {                                                // the window, then ONE rounding of the windowed sample
                const int64_t d = eq >= centre ? eq - centre : centre - eq;
                x[q] = x[q] * ((float)(step - d) / fstep);
            }
        }
        v[r] = {x[0], x[1]};
    }
    wave_real_spectrum(v, zs[w], tw, lane);
    if (!on) return;
    cf *dst = ws + (i * slots + slot) * FFT_N;
#pragma unroll
    for (int r = 0; r < 8; r++) dst[lane + 64 * r] = v[r];
}

// BLOCKS: the rows of output block m are the block table's range [first, last) in place of all rows of the clip
template <bool BLOCKS>
__global__ __launch_bounds__(SC_THREADS) void render_kernel(const scene_tables tb, const cf *__restrict__ spectra, int C, int L, int P,
                                                             int slots, const cf *__restrict__ ws, const float *ambient, float *out,
                                                             int64_t N, int64_t M)
{
    __shared__ cf ys[SC_CH][Z_LEN];
    __shared__ unsigned char inside[FFT_N];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t m = blockIdx.x, b = blockIdx.y;
    const int i_lo = BLOCKS ? tb.ranges[2 * (b * M + m)] : tb.ranges[b], i_hi = BLOCKS ? tb.ranges[2 * (b * M + m) + 1] : tb.ranges[b + 1];
    const int64_t *t_on = tb.rows + tb.n, *t_len = tb.rows + 2 * (int64_t)tb.n, *t_rir = tb.rows + 3 * (int64_t)tb.n;
    const int64_t n0 = FFT_N * m;

    // which samples of the block lie in some row's support (a support never reaches further than the block table's range covers)
    bool in0 = false, in1 = false;
    for (int i = i_lo; i < i_hi; i++) {
        const int64_t lo = t_on[i], hi = lo + t_len[i] + L - 1;
        in0 = in0 || (n0 + tid >= lo && n0 + tid < hi);
        in1 = in1 || (n0 + tid + 256 >= lo && n0 + tid + 256 < hi);
    }
    inside[tid] = in0;
    inside[tid + 256] = in1;
    if (!__syncthreads_or(in0 || in1)) {                       // a silent block: the ambient as it is
        for (int c = 0; c < C; c++)
            for (int q = 0; q < 2; q++) {
                const int64_t n = n0 + tid + 256 * q, idx = (b * C + c) * N + n;
                if (n < N) out[idx] = ambient ? ambient[idx] : 0.f;
            }
        return;
    }

    const cf *tw = spectra, *H = spectra + SC_TW;
    for (int c0 = 0; c0 < C; c0 += SC_CH) {
        const int nc = min(SC_CH, C - c0);
        cf acc[SC_CH][2];
#pragma unroll
        for (int c = 0; c < SC_CH; c++) acc[c][0] = acc[c][1] = {0.f, 0.f};
        for (int i = i_lo; i < i_hi; i++) {
            const int64_t o = t_on[i], len = t_len[i];
            const int64_t j0 = o >> 9, j1 = min(((o + len - 1) >> 9) + 1, M - 1);
            const int64_t p_lo = max((int64_t)0, m - j1), p_hi = min((int64_t)P - 1, m - j0);
            if (p_lo > p_hi) continue;
            const float g = tb.gains[i];
            const cf *Hi = H + (t_rir[i] * C + c0) * P * FFT_N + 2 * tid;
            const cf *Xi = ws + (int64_t)i * slots * FFT_N + 2 * tid;
            for (int64_t p = p_lo; p <= p_hi; p++) {
                const float4 xr = *reinterpret_cast<const float4 *>(Xi + (m - p - j0) * FFT_N);
                const cf x0 = {g * xr.x, g * xr.y}, x1 = {g * xr.z, g * xr.w};
#pragma unroll
                for (int c = 0; c < SC_CH; c++)
                    if (c < nc) {
                        const float4 hr = *reinterpret_cast<const float4 *>(Hi + ((int64_t)c * P + p) * FFT_N);
                        acc[c][0] = scene::spec_mac(acc[c][0], cf{hr.x, hr.y}, x0, tid == 0);
                        acc[c][1] = scene::spec_mac(acc[c][1], cf{hr.z, hr.w}, x1, false);
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < SC_CH; c++) {
            ys[c][zpad(2 * tid)] = acc[c][0];
            ys[c][zpad(2 * tid + 1)] = acc[c][1];
        }
        __syncthreads();
        for (int rd = 0; rd * SC_WAVES < nc; rd++) {           // a wave per channel, the inverse transform by conjugation
            const int c = w + SC_WAVES * rd;
            const bool on = c < nc;
            cf *z = ys[c];
            cf v[8];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const int k = lane + 64 * r;
                v[r] = salsa::cconj(scene::real_pack(z[zpad(k)], z[zpad((FFT_N - k) & (FFT_N - 1))], k, tw));
            }
            __syncthreads();
            wave_fft(v, z, tw, lane);
            if (on) {
                const int64_t row = (b * C + c0 + c) * N;
#pragma unroll
                for (int r = 4; r < 8; r++) {                  // samples 512 .. 1023 of the transform are block m
                    const int nl = 2 * (lane + 64 * r) - FFT_N;
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        const int64_t n = n0 + nl + q;
                        if (n < N) {
                            const float y = (q ? -v[r].im : v[r].re) * (1.f / FFT_N);
                            const float a = ambient ? ambient[row + n] : 0.f;
                            out[row + n] = inside[nl + q] ? a + y : a;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

__attribute__((format(printf, 2, 3))) int sfail(int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    salsa_set_last_error_(msg);                               // (copies the message)
    return code;
}

bool shape_ok(int R, int C, int L) { return R >= 1 && C >= 1 && C <= SC_MAX_CH && L >= 1 && L <= SC_MAX_RIR; }
int partitions(int L) { return (L + FFT_N - 1) / FFT_N; }
int64_t blocks_of(int64_t N) { return (N + FFT_N - 1) / FFT_N; }
// input blocks an event of max_len samples can meet at any onset, and never more than the clip has
int64_t slots_of(int64_t N, int max_len) { return std::min<int64_t>(((int64_t)max_len + FFT_N - 2) / FFT_N + 2, blocks_of(N)); }
// the workspace of n rows of at most max_len samples; 0 for what the launchers refuse
size_t workspace_bytes_of(int64_t n_samples, int max_len, int n)
{
    if (n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_len < 1 || n < 0) return 0;
    return (size_t)n * (size_t)slots_of(n_samples, max_len) * FFT_N * sizeof(cf);
}

// What the two render entry points differ in on the host: the words of their messages, the cap on a clip's rows, and whether the rows
// are segments -- six table rows with a ramp to check, and a block table that the render kernel takes its ranges from.
struct entry {
    const char *name, *row, *rows;
    int cap;
    bool segments;
};
constexpr entry ITEMS = {"salsa_scene_render", "an item", "items", SC_MAX_ITEMS, false};
constexpr entry SEGMENTS = {"salsa_scene_render_moving", "a segment", "segments", SC_MAX_SEGS, true};

// Both entry points.  Every table entry is checked on the host before the first device call (the CPU suite exercises these returns
// without a GPU); then the two launches.  `rows` is the (4, n) item or (6, n) segment table, `block_table` the host's copy for segments
// and unused for items, `ranges_dev` what scene_tables::ranges is: the device's clip_start for items, its block table for segments.
int render(const entry &en, const float *events, int64_t n_event_samples, const float *rir_spectra, int n_rirs, int n_channels, int rir_len,
           const int *clip_start, const int64_t *rows, const float *gains, const int *block_table, const int *ranges_dev,
           const int64_t *rows_dev, const float *gains_dev, int n_clips, int n, int max_len, const float *ambient, float *out,
           int64_t n_samples, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    if (!rir_spectra || ((uintptr_t)rir_spectra & 15) || !out || !clip_start || !ranges_dev || (en.segments && !block_table))
        return sfail(-1, "%s: null or unaligned pointer", en.name);
    if (!shape_ok(n_rirs, n_channels, rir_len)) return sfail(-1, "%s: 1 <= channels <= 16 and 1 <= rir length <= 16384", en.name);
    if (n_clips < 1 || n_clips > 65535 || n < 0 || n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_len < 1)
        return sfail(-1, "%s: bad sizes", en.name);
    if (n > 0 && (!events || !rows || !gains || !rows_dev || !gains_dev || !workspace || ((uintptr_t)workspace & 15) || n_event_samples < 1))
        return sfail(-1, "%s: null or unaligned pointer", en.name);
    if (clip_start[0] != 0 || clip_start[n_clips] != n) return sfail(-1, "%s: clip_start does not span the %s", en.name, en.rows);
    for (int b = 0; b < n_clips; b++)
        if (clip_start[b + 1] < clip_start[b] || clip_start[b + 1] - clip_start[b] > en.cap)
            return sfail(-1, "%s: clip_start must not decrease, and a clip holds at most %d %s", en.name, en.cap, en.rows);
    const int64_t M = blocks_of(n_samples), ns = n;
    const int P = partitions(rir_len);
    for (int b = 0; b < n_clips; b++) {
        const int *bt = en.segments ? block_table + 2 * (int64_t)b * M : nullptr;
        for (int64_t m = 0; bt && m < M; m++)
            if (bt[2 * m] < clip_start[b] || bt[2 * m] > bt[2 * m + 1] || bt[2 * m + 1] > clip_start[b + 1])
                return sfail(-1, "%s: a block's segment range lies outside its clip", en.name);
        for (int i = clip_start[b]; i < clip_start[b + 1]; i++) {
            const int64_t src = rows[i], o = rows[ns + i], len = rows[2 * ns + i], r = rows[3 * ns + i];
            if (len < 1 || len > max_len || src < 0 || src > n_event_samples - len)
                return sfail(-1, "%s: %s's samples lie outside the pool", en.name, en.row);
            if (o < 0 || o >= n_samples) return sfail(-1, "%s: an onset lies outside the clip", en.name);
            if (r < 0 || r >= n_rirs) return sfail(-1, "%s: %s names no response of the bank", en.name, en.row);
            if (!(fabsf(gains[i]) <= 3.4e38f)) return sfail(-1, "%s: a gain is not finite", en.name);
            if (!en.segments) continue;
            const int64_t centre = rows[4 * ns + i], step = rows[5 * ns + i];
            if (step != 0 && (step < SC_MIN_STEP || step > SC_MAX_STEP))
                return sfail(-1, "%s: a ramp step is 0 (no window) or 240 .. 16777216 samples", en.name);
            // |q - centre| < step for every sample 0 <= q < len: the ramp stays above zero inside the segment
            if (step != 0 && (centre <= -step || centre >= step || len - 1 - centre >= step))
                return sfail(-1, "%s: a ramp reaches zero or below inside its segment", en.name);
            const int64_t j0 = o >> 9, m_hi = std::min(std::min(((o + len - 1) >> 9) + 1, M - 1) + P - 1, M - 1);
            for (int64_t m = j0; m <= m_hi; m++)
                if (i < bt[2 * m] || i >= bt[2 * m + 1])
                    return sfail(-1, "%s: the block table leaves out a segment that reaches the block", en.name);
        }
    }
    if (workspace_bytes < workspace_bytes_of(n_samples, max_len, n)) return sfail(-5, "%s: workspace too small", en.name);
    const int slots = (int)slots_of(n_samples, max_len);
    if ((slots + SC_WAVES - 1) / SC_WAVES > 65535) return sfail(-1, "%s: %s is too long", en.name, en.row);
    const scene_tables tb = {ranges_dev, rows_dev, gains_dev, n};
    const cf *spectra = (const cf *)rir_spectra;
    const auto spectra_k = en.segments ? spectra_kernel<true> : spectra_kernel<false>;
    const auto render_k = en.segments ? render_kernel<true> : render_kernel<false>;
    if (n > 0)
        hipLaunchKernelGGL(spectra_k, dim3((unsigned)n, (unsigned)((slots + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS), 0, stream, events, tb,
                           slots, M, spectra, (cf *)workspace);
    hipLaunchKernelGGL(render_k, dim3((unsigned)M, (unsigned)n_clips), dim3(SC_THREADS), 0, stream, tb, spectra, n_channels, rir_len, P, slots,
                       (const cf *)workspace, ambient, out, n_samples, M);
    return hipGetLastError() == hipSuccess ? 0 : sfail(-6, "%s: launch failed", en.name);
}

} // namespace

extern "C" size_t salsa_scene_rir_spectra_bytes(int n_rirs, int n_channels, int rir_len)
{
    if (!shape_ok(n_rirs, n_channels, rir_len)) return 0;
    return ((size_t)SC_TW + (size_t)n_rirs * n_channels * partitions(rir_len) * FFT_N) * sizeof(cf);
}

extern "C" int salsa_scene_rir_spectra(const float *rirs, int n_rirs, int n_channels, int rir_len, float *spectra, void *hip_stream)
{
    if (!rirs || !spectra || ((uintptr_t)spectra & 15)) return sfail(-1, "salsa_scene_rir_spectra: null or unaligned pointer");
    if (!shape_ok(n_rirs, n_channels, rir_len)) return sfail(-1, "salsa_scene_rir_spectra: 1 <= channels <= 16 and 1 <= length <= 16384");
    const int P = partitions(rir_len);
    const int64_t units = (int64_t)n_rirs * n_channels * P;
    if ((units + SC_WAVES - 1) / SC_WAVES > 0x7fffffff) return sfail(-1, "salsa_scene_rir_spectra: too many responses");
    hipLaunchKernelGGL(twiddle_kernel, dim3(SC_TW / 256), dim3(256), 0, (hipStream_t)hip_stream, (cf *)spectra);
    hipLaunchKernelGGL(rir_spectra_kernel, dim3((unsigned)((units + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS), 0, (hipStream_t)hip_stream,
                       rirs, units, rir_len, P, (cf *)spectra);
    return hipGetLastError() == hipSuccess ? 0 : sfail(-6, "salsa_scene_rir_spectra: launch failed");
}

extern "C" size_t salsa_scene_workspace_bytes(int64_t n_samples, int max_event_len, int n_items)
{
    return workspace_bytes_of(n_samples, max_event_len, n_items);
}

extern "C" int salsa_scene_render(const float *events, int64_t n_event_samples, const float *rir_spectra, int n_rirs, int n_channels,
                                  int rir_len, const int *clip_start, const int64_t *items, const float *gains,
                                  const int *clip_start_dev, const int64_t *items_dev, const float *gains_dev, int n_clips, int n_items,
                                  int max_event_len, const float *ambient, float *out, int64_t n_samples, void *workspace,
                                  size_t workspace_bytes, void *hip_stream)
{
    return render(ITEMS, events, n_event_samples, rir_spectra, n_rirs, n_channels, rir_len, clip_start, items, gains, nullptr, clip_start_dev,
                  items_dev, gains_dev, n_clips, n_items, max_event_len, ambient, out, n_samples, workspace, workspace_bytes,
                  (hipStream_t)hip_stream);
}

// ---- moving sources: segments and a block table in place of items
extern "C" size_t salsa_scene_moving_workspace_bytes(int64_t n_samples, int max_segment_len, int n_segments)
{
    return workspace_bytes_of(n_samples, max_segment_len, n_segments);
}

extern "C" int salsa_scene_render_moving(const float *events, int64_t n_event_samples, const float *rir_spectra, int n_rirs, int n_channels,
                                         int rir_len, const int *clip_start, const int64_t *segments, const float *gains,
                                         const int *block_table, const int64_t *segments_dev, const float *gains_dev,
                                         const int *block_table_dev, int n_clips, int n_segments, int max_segment_len,
                                         const float *ambient, float *out, int64_t n_samples, void *workspace, size_t workspace_bytes,
                                         void *hip_stream)
{
    return render(SEGMENTS, events, n_event_samples, rir_spectra, n_rirs, n_channels, rir_len, clip_start, segments, gains, block_table,
                  block_table_dev, segments_dev, gains_dev, n_clips, n_segments, max_segment_len, ambient, out, n_samples, workspace,
                  workspace_bytes, (hipStream_t)hip_stream);
}
