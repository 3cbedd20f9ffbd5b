// scene_render.hip -- labelled SELD scenes rendered on the device (include/salsa_hip.h: salsa_scene_*):
//   audio[b, c, n] = ambient[b, c, n] + sum_i g_i (h[r_i, c, :] * s_i)[n - o_i]        0 <= n < N, `*` the full linear convolution
// by uniformly partitioned overlap-save in float32.  A partition is 512 samples; the real 1024-point transform of two neighbouring
// partitions is a 512-point complex FFT, one wave with 8 points per lane (scene_fft.h has the per-lane arithmetic and the packed
// half-spectrum layout).  The clip has ONE block grid, output block m = samples [512 m, 512 (m + 1)); an item is laid onto that grid
// at its onset before it is transformed, so onsets need no alignment.
//
//   rir_spectra_kernel     once per bank: h[r, c, 512 p .. 512 p + 511] followed by 512 zeros -> H[r, c, p][k], behind the twiddle table
//   item_spectra_kernel    per item and input block j (samples [512 (j - 1), 512 (j + 1)) of the item on the clip's grid, only the
//                          blocks the dry event meets) -> X_i[j][k] in the caller's workspace
//   render_kernel          per (clip, output block m), one workgroup for all channels: Y_c[k] = sum_i sum_p g_i H[r_i, c, p][k]
//                          X_i[m - p][k] with items and partitions in ascending order, the inverse transform per channel, whose last 512
//                          samples are block m, then ambient + y where a sample lies in some item's support [o_i, o_i + len_i + L - 1)
//                          and the ambient's own bits (or zero) everywhere else, so that silence stays silent.
// Nothing is summed across workgroups: no atomics, one fixed order, so two runs agree bit for bit and a clip does not depend on the
// rest of its batch.  All offsets are 64-bit.  The launchers check everything on the host before the first device call.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
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

struct scene_tables {
    const int *clip_start;      // (B + 1)
    const int64_t *items;       // (4, n_items): source offset in `events`, onset, length, rir
    const float *gains;         // (n_items)
    int n_items;
};

__global__ __launch_bounds__(SC_THREADS) void item_spectra_kernel(const float *__restrict__ events, const scene_tables tb, int slots,
                                                                   int64_t M, const cf *__restrict__ tw, cf *__restrict__ ws)
{
    __shared__ cf zs[SC_WAVES][Z_LEN];
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int64_t i = blockIdx.x;
    const int64_t src = tb.items[i], o = tb.items[tb.n_items + i], len = tb.items[2 * (int64_t)tb.n_items + i];
    const int64_t j0 = o >> 9, j1 = min(((o + len - 1) >> 9) + 1, M - 1);
    const int slot = (int)blockIdx.y * SC_WAVES + w;
    const int64_t j = j0 + slot;
    const bool on = slot < slots && j <= j1;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t e = FFT_N * (j - 1) + 2 * (lane + 64 * r) - o;      // index into the dry event
        v[r] = {on && e >= 0 && e < len ? events[src + e] : 0.f, on && e + 1 >= 0 && e + 1 < len ? events[src + e + 1] : 0.f};
    }
    wave_real_spectrum(v, zs[w], tw, lane);
    if (!on) return;
    cf *dst = ws + (i * slots + slot) * FFT_N;
#pragma unroll
    for (int r = 0; r < 8; r++) dst[lane + 64 * r] = v[r];
}

__global__ __launch_bounds__(SC_THREADS) void render_kernel(const scene_tables tb, const cf *__restrict__ spectra, int C, int L, int P,
                                                             int slots, const cf *__restrict__ ws, const float *ambient, float *out,
                                                             int64_t N, int64_t M)
{
    __shared__ cf ys[SC_CH][Z_LEN];
    __shared__ unsigned char inside[FFT_N];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t m = blockIdx.x, b = blockIdx.y;
    const int i_lo = tb.clip_start[b], i_hi = tb.clip_start[b + 1];
    const int64_t *t_on = tb.items + tb.n_items, *t_len = tb.items + 2 * (int64_t)tb.n_items, *t_rir = tb.items + 3 * (int64_t)tb.n_items;
    const int64_t n0 = FFT_N * m;

    // which samples of the block lie in some item's support
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

// ---- moving sources: the host has cut every item into segments, one per trajectory node; a segment is an
// item of its own response whose dry samples are weighted by a linear ramp while they are loaded.  A static item is ONE segment of
// step 0, loaded as it is, so a batch of static items goes through the arithmetic of the kernels above in the same order.
struct moving_tables {
    const int *block_tab;       // (B, M, 2): first and one-past-last segment that can reach output block m of clip b
    const int64_t *segs;        // (6, n_segs): source offset in `events`, onset, length, rir, ramp centre from the segment's start, ramp step
    const float *gains;         // (n_segs)
    int n_segs;
};

__global__ __launch_bounds__(SC_THREADS) void segment_spectra_kernel(const float *__restrict__ events, const moving_tables tb, int slots,
                                                                      int64_t M, const cf *__restrict__ tw, cf *__restrict__ ws)
{
    __shared__ cf zs[SC_WAVES][Z_LEN];
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int64_t i = blockIdx.x, n = tb.n_segs;
    const int64_t src = tb.segs[i], o = tb.segs[n + i], len = tb.segs[2 * n + i], centre = tb.segs[4 * n + i], step = tb.segs[5 * n + i];
    const int64_t j0 = o >> 9, j1 = min(((o + len - 1) >> 9) + 1, M - 1);
    const int slot = (int)blockIdx.y * SC_WAVES + w;
    const int64_t j = j0 + slot;
    const bool on = slot < slots && j <= j1;
    const float fstep = (float)step;
    cf v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int64_t e = FFT_N * (j - 1) + 2 * (lane + 64 * r) - o;      // index into the segment's dry samples
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

// render_kernel with the segments of the block table's range [first, last) in place of all items of the clip
__global__ __launch_bounds__(SC_THREADS) void render_moving_kernel(const moving_tables tb, const cf *__restrict__ spectra, int C, int L,
                                                                    int P, int slots, const cf *__restrict__ ws, const float *ambient,
                                                                    float *out, int64_t N, int64_t M)
{
    __shared__ cf ys[SC_CH][Z_LEN];
    __shared__ unsigned char inside[FFT_N];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t m = blockIdx.x, b = blockIdx.y;
    const int i_lo = tb.block_tab[2 * (b * M + m)], i_hi = tb.block_tab[2 * (b * M + m) + 1];
    const int64_t *t_on = tb.segs + tb.n_segs, *t_len = tb.segs + 2 * (int64_t)tb.n_segs, *t_rir = tb.segs + 3 * (int64_t)tb.n_segs;
    const int64_t n0 = FFT_N * m;

    // which samples of the block lie in some segment's support (a support never reaches further than the range covers)
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

int sfail(int code, const char *msg)
{
    salsa_set_last_error_(msg);
    return code;
}

bool shape_ok(int R, int C, int L) { return R >= 1 && C >= 1 && C <= SC_MAX_CH && L >= 1 && L <= SC_MAX_RIR; }
int partitions(int L) { return (L + FFT_N - 1) / FFT_N; }
int64_t blocks_of(int64_t N) { return (N + FFT_N - 1) / FFT_N; }
// input blocks an event of max_len samples can meet at any onset, and never more than the clip has
int64_t slots_of(int64_t N, int max_len) { return std::min<int64_t>(((int64_t)max_len + FFT_N - 2) / FFT_N + 2, blocks_of(N)); }

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
    if (n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_event_len < 1 || n_items < 0) return 0;
    return (size_t)n_items * (size_t)slots_of(n_samples, max_event_len) * FFT_N * sizeof(cf);
}

extern "C" int salsa_scene_render(const float *events, int64_t n_event_samples, const float *rir_spectra, int n_rirs, int n_channels,
                                  int rir_len, const int *clip_start, const int64_t *items, const float *gains,
                                  const int *clip_start_dev, const int64_t *items_dev, const float *gains_dev, int n_clips, int n_items,
                                  int max_event_len, const float *ambient, float *out, int64_t n_samples, void *workspace,
                                  size_t workspace_bytes, void *hip_stream)
{
    // everything is checked on the host tables before the first device call (the CPU suite exercises these returns without a GPU)
    if (!rir_spectra || ((uintptr_t)rir_spectra & 15) || !out || !clip_start || !clip_start_dev)
        return sfail(-1, "salsa_scene_render: null or unaligned pointer");
    if (!shape_ok(n_rirs, n_channels, rir_len)) return sfail(-1, "salsa_scene_render: 1 <= channels <= 16 and 1 <= rir length <= 16384");
    if (n_clips < 1 || n_clips > 65535 || n_items < 0 || n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_event_len < 1)
        return sfail(-1, "salsa_scene_render: bad sizes");
    if (n_items > 0 && (!events || !items || !gains || !items_dev || !gains_dev || !workspace || ((uintptr_t)workspace & 15) || n_event_samples < 1))
        return sfail(-1, "salsa_scene_render: null or unaligned pointer");
    if (clip_start[0] != 0 || clip_start[n_clips] != n_items) return sfail(-1, "salsa_scene_render: clip_start does not span the items");
    for (int b = 0; b < n_clips; b++)
        if (clip_start[b + 1] < clip_start[b] || clip_start[b + 1] - clip_start[b] > SC_MAX_ITEMS)
            return sfail(-1, "salsa_scene_render: clip_start must not decrease, and a clip holds at most 256 items");
    for (int i = 0; i < n_items; i++) {
        const int64_t src = items[i], o = items[(int64_t)n_items + i], len = items[2 * (int64_t)n_items + i], r = items[3 * (int64_t)n_items + i];
        if (len < 1 || len > max_event_len || src < 0 || src > n_event_samples - len) return sfail(-1, "salsa_scene_render: an item's event lies outside the pool");
        if (o < 0 || o >= n_samples) return sfail(-1, "salsa_scene_render: an onset lies outside the clip");
        if (r < 0 || r >= n_rirs) return sfail(-1, "salsa_scene_render: an item names no response of the bank");
        if (!(fabsf(gains[i]) <= 3.4e38f)) return sfail(-1, "salsa_scene_render: a gain is not finite");
    }
    if (workspace_bytes < salsa_scene_workspace_bytes(n_samples, max_event_len, n_items)) return sfail(-5, "salsa_scene_render: workspace too small");
    const int64_t M = blocks_of(n_samples);
    const int slots = (int)slots_of(n_samples, max_event_len), P = partitions(rir_len);
    if ((slots + SC_WAVES - 1) / SC_WAVES > 65535) return sfail(-1, "salsa_scene_render: event too long");
    const scene_tables tb = {clip_start_dev, items_dev, gains_dev, n_items};
    const cf *spectra = (const cf *)rir_spectra;
    if (n_items > 0)
        hipLaunchKernelGGL(item_spectra_kernel, dim3((unsigned)n_items, (unsigned)((slots + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS), 0,
                           (hipStream_t)hip_stream, events, tb, slots, M, spectra, (cf *)workspace);
    hipLaunchKernelGGL(render_kernel, dim3((unsigned)M, (unsigned)n_clips), dim3(SC_THREADS), 0, (hipStream_t)hip_stream, tb, spectra,
                       n_channels, rir_len, P, slots, (const cf *)workspace, ambient, out, n_samples, M);
    return hipGetLastError() == hipSuccess ? 0 : sfail(-6, "salsa_scene_render: launch failed");
}

// ---- moving sources: segments and a block table in place of items
namespace {
constexpr int SC_MAX_SEGS = 65536;                  // segments per clip
constexpr int64_t SC_MIN_STEP = 240, SC_MAX_STEP = 1 << 24;   // ramp steps; up to 2^24 the window's numerator is exact in float32
} // namespace

extern "C" size_t salsa_scene_moving_workspace_bytes(int64_t n_samples, int max_segment_len, int n_segments)
{
    if (n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_segment_len < 1 || n_segments < 0) return 0;
    return (size_t)n_segments * (size_t)slots_of(n_samples, max_segment_len) * FFT_N * sizeof(cf);
}

extern "C" int salsa_scene_render_moving(const float *events, int64_t n_event_samples, const float *rir_spectra, int n_rirs, int n_channels,
                                         int rir_len, const int *clip_start, const int64_t *segments, const float *gains,
                                         const int *block_table, const int64_t *segments_dev, const float *gains_dev,
                                         const int *block_table_dev, int n_clips, int n_segments, int max_segment_len,
                                         const float *ambient, float *out, int64_t n_samples, void *workspace, size_t workspace_bytes,
                                         void *hip_stream)
{
    // as salsa_scene_render: every table entry is checked on the host before the first device call
    if (!rir_spectra || ((uintptr_t)rir_spectra & 15) || !out || !clip_start || !block_table || !block_table_dev)
        return sfail(-1, "salsa_scene_render_moving: null or unaligned pointer");
    if (!shape_ok(n_rirs, n_channels, rir_len))
        return sfail(-1, "salsa_scene_render_moving: 1 <= channels <= 16 and 1 <= rir length <= 16384");
    if (n_clips < 1 || n_clips > 65535 || n_segments < 0 || n_samples < 1 || blocks_of(n_samples) > 0x7fffffff || max_segment_len < 1)
        return sfail(-1, "salsa_scene_render_moving: bad sizes");
    if (n_segments > 0 && (!events || !segments || !gains || !segments_dev || !gains_dev || !workspace || ((uintptr_t)workspace & 15) || n_event_samples < 1))
        return sfail(-1, "salsa_scene_render_moving: null or unaligned pointer");
    if (clip_start[0] != 0 || clip_start[n_clips] != n_segments)
        return sfail(-1, "salsa_scene_render_moving: clip_start does not span the segments");
    for (int b = 0; b < n_clips; b++)
        if (clip_start[b + 1] < clip_start[b] || clip_start[b + 1] - clip_start[b] > SC_MAX_SEGS)
            return sfail(-1, "salsa_scene_render_moving: clip_start must not decrease, and a clip holds at most 65536 segments");
    const int64_t M = blocks_of(n_samples), ns = n_segments;
    const int P = partitions(rir_len);
    for (int b = 0; b < n_clips; b++) {
        const int *bt = block_table + 2 * (int64_t)b * M;
        for (int64_t m = 0; m < M; m++)
            if (bt[2 * m] < clip_start[b] || bt[2 * m] > bt[2 * m + 1] || bt[2 * m + 1] > clip_start[b + 1])
                return sfail(-1, "salsa_scene_render_moving: a block's segment range lies outside its clip");
        for (int i = clip_start[b]; i < clip_start[b + 1]; i++) {
            const int64_t src = segments[i], o = segments[ns + i], len = segments[2 * ns + i], r = segments[3 * ns + i],
                          centre = segments[4 * ns + i], step = segments[5 * ns + i];
            if (len < 1 || len > max_segment_len || src < 0 || src > n_event_samples - len)
                return sfail(-1, "salsa_scene_render_moving: a segment's samples lie outside the pool");
            if (o < 0 || o >= n_samples) return sfail(-1, "salsa_scene_render_moving: an onset lies outside the clip");
            if (r < 0 || r >= n_rirs) return sfail(-1, "salsa_scene_render_moving: a segment names no response of the bank");
            if (!(fabsf(gains[i]) <= 3.4e38f)) return sfail(-1, "salsa_scene_render_moving: a gain is not finite");
            if (step != 0 && (step < SC_MIN_STEP || step > SC_MAX_STEP))
                return sfail(-1, "salsa_scene_render_moving: a ramp step is 0 (no window) or 240 .. 16777216 samples");
            // |q - centre| < step for every sample 0 <= q < len: the ramp stays above zero inside the segment
            if (step != 0 && (centre <= -step || centre >= step || len - 1 - centre >= step))
                return sfail(-1, "salsa_scene_render_moving: a ramp reaches zero or below inside its segment");
            const int64_t j0 = o >> 9, m_hi = std::min(std::min(((o + len - 1) >> 9) + 1, M - 1) + P - 1, M - 1);
            for (int64_t m = j0; m <= m_hi; m++)
                if (i < bt[2 * m] || i >= bt[2 * m + 1])
                    return sfail(-1, "salsa_scene_render_moving: the block table leaves out a segment that reaches the block");
        }
    }
    if (workspace_bytes < salsa_scene_moving_workspace_bytes(n_samples, max_segment_len, n_segments))
        return sfail(-5, "salsa_scene_render_moving: workspace too small");
    const int slots = (int)slots_of(n_samples, max_segment_len);
    if ((slots + SC_WAVES - 1) / SC_WAVES > 65535) return sfail(-1, "salsa_scene_render_moving: segment too long");
    const moving_tables tb = {block_table_dev, segments_dev, gains_dev, n_segments};
    const cf *spectra = (const cf *)rir_spectra;
    if (n_segments > 0)
        hipLaunchKernelGGL(segment_spectra_kernel, dim3((unsigned)n_segments, (unsigned)((slots + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS),
                           0, (hipStream_t)hip_stream, events, tb, slots, M, spectra, (cf *)workspace);
    hipLaunchKernelGGL(render_moving_kernel, dim3((unsigned)M, (unsigned)n_clips), dim3(SC_THREADS), 0, (hipStream_t)hip_stream, tb, spectra,
                       n_channels, rir_len, P, slots, (const cf *)workspace, ambient, out, n_samples, M);
    return hipGetLastError() == hipSuccess ? 0 : sfail(-6, "salsa_scene_render_moving: launch failed");
}
