// rir_decay.hip -- energy decay curve and room-acoustic parameters of a bank of impulse responses (include/salsa_hip.h:
// salsa_rir_decay; salsa_amd/rooms.py: rir_acoustics).  Per (response, channel), all in float64:
//     e[n] = (double)h[n]^2,  EDC[n] = sum_{m >= n} e[m],  E = EDC[0],  n_d = first argmax |h|,
//     i(x) = first n with EDC[n] <= E f_x   (f_x = 10^(x / 10) from the host: no device logarithm decides an index),
//     EDT, T20, T30 = -60 / slope of the least-squares line through (n / fs, 10 log10(EDC[n] / E)), n in [i(lo), i(hi)],
//     headroom = -slope per tap x (L - 1 - i(hi)),  DRR and C50 from sums of e over tap ranges around n_d.
//
//   decay_kernel<STRIDE>   ONE workgroup of 256 threads per (response, channel); thread t owns the P = ceil(L / 256) consecutive
//                          taps t P .. t P + P - 1.  The response is loaded once, coalesced (lane = consecutive tap), into LDS as
//                          float32 and stays there: row t of the LDS array is thread t's run, the row stride is ODD (P | 1 <= STRIDE),
//                          so that the 64 lanes of a wave, which read the same column of 64 different rows, fall into 64 different
//                          banks (stride 33 or 65 dwords over 64 banks: a permutation).  Every later pass walks the thread's own row.
//                          The curve is not kept: a pass that needs EDC[n] rebuilds the thread-local suffix sum s from the row (one
//                          float64 multiply-add per tap, the same operations in the same order, hence the same bits every time) and
//                          forms EDC[n] = off_t + s.  A register copy would need the run length as a compile-time constant and 128
//                          VGPRs for 64 float64 values; an LDS copy of the float64 curve is 128 KiB at 16384 taps, more than half of a
//                          CU's 160 KiB.  The float32 row costs 33 KiB (L <= 8192: four workgroups per CU) or 65 KiB (two).
//
// Order of every sum (fixed: two calls give equal bits, and nothing depends on the grid or on the other responses):
//   * thread-local suffix sums run from the thread's last tap down to its first, from 0;
//   * off_t = sum of the totals of the threads u > t, added one by one from u = 255 down (every thread walks the 256 totals in LDS
//     itself, reading one address per step: a broadcast), so off_t = fl(off_{t+1} + total_{t+1}) and E = fl(off_0 + total_0);
//     EDC[n] = fl(off_t + s[n]) therefore never increases with n, also across threads, and a crossing i(x) is a COUNT: the number
//     of taps with EDC[n] > E f_x, integers summed over the threads;
//   * every other sum is a thread-local sum in a fixed tap order (window energies over ascending taps, fit means and moments over
//     descending ones, beside the suffix sum they need), then a tree over the lanes of a wave (shuffle down by 32, 16, .., 1), then
//     the four waves' values added in wave order.
// No atomics.  The launcher checks every argument on the host before the first device call; all offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int DK_THREADS = 256, DK_WAVES = 4;
constexpr int DK_MAX_RIR = 16384, DK_MAX_CHANNELS = 16, DK_MAX_RIRS = 65535;
constexpr int DK_LEVELS = 5;                                  // 0, -5, -10, -25, -35 dB
constexpr int DK_FITS = 3;                                    // EDT (0, -10), T20 (-5, -25), T30 (-5, -35): indices into the levels

struct decay_args {
    double factor[DK_LEVELS];                                 // 10^(x / 10)
    double fs;
    int rir_len, run, halfwidth, early;                       // run = P; early = round(0.05 fs) taps
};

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                                 // lane 0 holds the sum
}

// the sum of v over the workgroup in a fixed order, returned to every thread; s_red has DK_WAVES entries
__device__ inline double block_sum(double v, double *s_red, int lane, int w)
{
    v = wave_sum(v);
    __syncthreads();                                          // the previous use of s_red is over
    if (lane == 0) s_red[w] = v;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int u = 1; u < DK_WAVES; u++) t += s_red[u];
    return t;
}

__device__ inline int block_sum_int(int v, int *s_red, int lane, int w)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();
    if (lane == 0) s_red[w] = v;
    __syncthreads();
    int t = s_red[0];
#pragma unroll
    for (int u = 1; u < DK_WAVES; u++) t += s_red[u];
    return t;
}

template <int STRIDE>
__global__ __launch_bounds__(DK_THREADS) void decay_kernel(const float *__restrict__ rirs, const decay_args a, double *__restrict__ params,
                                                           double *__restrict__ edc)
{
    __shared__ float s_h[DK_THREADS * STRIDE];
    __shared__ double s_tot[DK_THREADS];
    __shared__ double s_red[DK_WAVES];
    __shared__ float s_pk[DK_WAVES];
    __shared__ int s_pi[DK_WAVES], s_redi[DK_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int L = a.rir_len, P = a.run, stride = P | 1;       // stride <= STRIDE (the launcher picks the instantiation)
    const int64_t rc = (int64_t)blockIdx.x;
    const float *h = rirs + rc * L;
    const int first = tid * P, last = min(first + P, L);      // my taps [first, last); empty for the threads past the end
    float *row = s_h + tid * stride;

    // coalesced load into the rows
    for (int i = tid; i < L; i += DK_THREADS) s_h[(i / P) * stride + (i % P)] = h[i];
    __syncthreads();

    // thread-local total and peak (the first index of the largest |h|)
    double tot = 0.0;
    float pk = -1.f;
    int pi = 0;
    for (int n = last - 1; n >= first; n--) {
        const float v = row[n - first];
        const double d = (double)v;
        tot += d * d;
        if (fabsf(v) >= pk) { pk = fabsf(v); pi = n; }        // descending n and >=: the smallest index of the largest value
    }
    s_tot[tid] = tot;
    // the peak over the wave, then over the waves: larger value wins, equal values go to the smaller index (exact, any order)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_down(pk, d, 64);
        const int oi = __shfl_down(pi, d, 64);
        if (ov > pk || (ov == pk && oi < pi)) { pk = ov; pi = oi; }
    }
    if (lane == 0) { s_pk[w] = pk; s_pi[w] = pi; }
    __syncthreads();
    pk = s_pk[0];
    pi = s_pi[0];
#pragma unroll
    for (int u = 1; u < DK_WAVES; u++)
        if (s_pk[u] > pk || (s_pk[u] == pk && s_pi[u] < pi)) { pk = s_pk[u]; pi = s_pi[u]; }
    const int n_d = pk > 0.f ? pi : 0;                        // (a thread without taps carries pk = -1)

    // suffix scan of the threads' totals, from the last thread down, the same chain in every thread
    double off = 0.0, E = 0.0;
    for (int u = DK_THREADS - 1; u >= 0; u--) {
        if (u == tid) off = E;
        E += s_tot[u];
    }

    double *out = params + rc * SALSA_DECAY_PARAMS;
    if (!(E > 0.0)) {                                         // a silent response: energy 0, peak 0, the rest NaN
        if (tid < SALSA_DECAY_PARAMS) out[tid] = tid == SALSA_DECAY_ENERGY || tid == SALSA_DECAY_PEAK ? 0.0 : (double)NAN;
        if (edc)
            for (int n = first; n < last; n++) edc[rc * L + n] = 0.0;
        return;
    }

    // crossings as counts; the curve's store; the window energies
    double thr[DK_LEVELS];
#pragma unroll
    for (int k = 0; k < DK_LEVELS; k++) thr[k] = E * a.factor[k];
    int cnt[DK_LEVELS], cpos = 0;
#pragma unroll
    for (int k = 0; k < DK_LEVELS; k++) cnt[k] = 0;
    const int d_lo = n_d - a.halfwidth, d_hi = n_d + a.halfwidth, n_e = n_d + a.early;    // direct: [d_lo, d_hi]; early: n < n_e
    double e_dir = 0.0, e_rest = 0.0, e_early = 0.0, e_late = 0.0;
    {
        double s = 0.0;
        for (int n = last - 1; n >= first; n--) {
            const double d = (double)row[n - first];
            s += d * d;
            const double c = off + s;
#pragma unroll
            for (int k = 0; k < DK_LEVELS; k++) cnt[k] += c > thr[k] ? 1 : 0;
            cpos += c > 0.0 ? 1 : 0;
            if (edc) edc[rc * L + n] = c;
        }
        for (int n = first; n < last; n++) {
            const double d = (double)row[n - first], e = d * d;
            if (n >= d_lo && n <= d_hi) e_dir += e; else e_rest += e;
            if (n < n_e) e_early += e; else e_late += e;
        }
    }
    int cross[DK_LEVELS];
#pragma unroll
    for (int k = 0; k < DK_LEVELS; k++) cross[k] = block_sum_int(cnt[k], s_redi, lane, w);   // i(x), or L: no crossing
    cpos = block_sum_int(cpos, s_redi, lane, w);              // EDC[n] > 0 exactly for n < cpos
    e_dir = block_sum(e_dir, s_red, lane, w);
    e_rest = block_sum(e_rest, s_red, lane, w);
    e_early = block_sum(e_early, s_red, lane, w);
    e_late = block_sum(e_late, s_red, lane, w);

    // the three fits: mean first, then deviations
    const int fit_lo[DK_FITS] = {0, 1, 1}, fit_hi[DK_FITS] = {2, 3, 4};
    double T[DK_FITS], room[DK_FITS];
#pragma unroll
    for (int f = 0; f < DK_FITS; f++) {
        const int i0 = cross[fit_lo[f]], i1 = cross[fit_hi[f]];
        T[f] = room[f] = (double)NAN;
        if (i1 >= L || i1 >= cpos || i1 - i0 + 1 < 2) continue;                            // uniform over the workgroup
        const int b0 = max(first, i0), b1 = min(last - 1, i1);                             // my part of the range [b0, b1]
        const double count = (double)(i1 - i0 + 1), nbar = 0.5 * ((double)i0 + (double)i1);
        double sd = 0.0;
        if (b0 <= b1) {
            double s = 0.0;
            for (int n = last - 1; n > b1; n--) { const double d = (double)row[n - first]; s += d * d; }
            // descending taps rebuild s; the level sum itself is formed over descending taps too (a fixed order all the same)
            for (int n = b1; n >= b0; n--) {
                const double d = (double)row[n - first];
                s += d * d;
                sd += 10.0 * log10((off + s) / E);
            }
        }
        const double dbar = block_sum(sd, s_red, lane, w) / count;
        double sxy = 0.0, sxx = 0.0;
        if (b0 <= b1) {
            double s = 0.0;
            for (int n = last - 1; n > b1; n--) { const double d = (double)row[n - first]; s += d * d; }
            for (int n = b1; n >= b0; n--) {
                const double d = (double)row[n - first];
                s += d * d;
                const double x = (double)n - nbar, y = 10.0 * log10((off + s) / E) - dbar;
                sxy += x * y;
                sxx += x * x;
            }
        }
        sxy = block_sum(sxy, s_red, lane, w);
        sxx = block_sum(sxx, s_red, lane, w);
        const double slope = sxy / sxx;                                                    // dB per tap
        T[f] = -60.0 / (slope * a.fs);
        room[f] = -slope * (double)(L - 1 - i1);
    }

    if (tid == 0) {
        out[SALSA_DECAY_ENERGY] = E;
        out[SALSA_DECAY_PEAK] = (double)n_d;
        out[SALSA_DECAY_EDT] = T[0];
        out[SALSA_DECAY_T20] = T[1];
        out[SALSA_DECAY_T30] = T[2];
        out[SALSA_DECAY_HEADROOM_EDT] = room[0];
        out[SALSA_DECAY_HEADROOM_T20] = room[1];
        out[SALSA_DECAY_HEADROOM_T30] = room[2];
        out[SALSA_DECAY_DRR_DB] = e_rest > 0.0 ? 10.0 * log10(e_dir / e_rest) : (double)INFINITY;
        out[SALSA_DECAY_C50_DB] = e_late > 0.0 ? 10.0 * log10(e_early / e_late) : (double)INFINITY;
#pragma unroll
        for (int k = 0; k < DK_LEVELS; k++) out[SALSA_DECAY_CROSS_0DB + k] = cross[k] < L ? (double)cross[k] : (double)NAN;
    }
}

__attribute__((format(printf, 2, 3))) int dfail(int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    salsa_set_last_error_(msg);
    return code;
}

} // namespace

extern "C" int salsa_rir_decay_params(void) { return SALSA_DECAY_PARAMS; }

extern "C" int salsa_rir_decay(const float *d_rirs, int n_rirs, int n_channels, int rir_len, double fs, int direct_halfwidth,
                               double *d_params, double *d_edc, void *hip_stream)
{
    if (!d_rirs || !d_params) return dfail(-1, "salsa_rir_decay: null pointer");
    if (n_rirs < 1 || n_rirs > DK_MAX_RIRS) return dfail(-1, "salsa_rir_decay: 1 .. %d responses", DK_MAX_RIRS);
    if (n_channels < 1 || n_channels > DK_MAX_CHANNELS) return dfail(-1, "salsa_rir_decay: 1 .. %d channels", DK_MAX_CHANNELS);
    if (rir_len < 1 || rir_len > DK_MAX_RIR) return dfail(-1, "salsa_rir_decay: 1 <= rir length <= %d", DK_MAX_RIR);
    if (!(fs > 0.0 && fs <= 1e9)) return dfail(-1, "salsa_rir_decay: fs must be positive and at most 1e9");
    if (direct_halfwidth < 0 || direct_halfwidth > DK_MAX_RIR) return dfail(-1, "salsa_rir_decay: 0 <= direct_halfwidth <= %d", DK_MAX_RIR);
    static const double level_db[DK_LEVELS] = {0.0, -5.0, -10.0, -25.0, -35.0};
    decay_args a;
    for (int k = 0; k < DK_LEVELS; k++) a.factor[k] = pow(10.0, level_db[k] / 10.0);
    a.fs = fs;
    a.rir_len = rir_len;
    a.run = (rir_len + DK_THREADS - 1) / DK_THREADS;          // 1 .. 64
    a.halfwidth = direct_halfwidth;
    a.early = (int)floor(0.05 * fs + 0.5);
    const dim3 grid((unsigned)(n_rirs * n_channels));         // <= 65535 x 16
    if ((a.run | 1) <= 33)
        hipLaunchKernelGGL(decay_kernel<33>, grid, dim3(DK_THREADS), 0, (hipStream_t)hip_stream, d_rirs, a, d_params, d_edc);
    else
        hipLaunchKernelGGL(decay_kernel<65>, grid, dim3(DK_THREADS), 0, (hipStream_t)hip_stream, d_rirs, a, d_params, d_edc);
    return hipGetLastError() == hipSuccess ? 0 : dfail(-6, "salsa_rir_decay: launch failed");
}
