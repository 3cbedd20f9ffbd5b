// doa_hist.hip -- a model-free localiser on the SALSA features' directional channels (include/salsa_hip.h: salsa_doa_hist,
// salsa_doa_hist_supported, salsa_doa_hist_cells, salsa_doa_hist_limits; salsa_amd/localize.py).  The reference
// has no counterpart: the definition is this project's.
// Channels 4-6 of a feature map hold one direction estimate per time-frequency bin.  For a label frame f (P feature frames) the cells
// (t, col), P f <= t < P (f + 1), col0 <= col < col1, t ascending then col ascending, each cast at most one vote:
//     v = (ch4, ch5, ch6);  no vote when v is all zero (either sign) or holds a non-finite value
//     FOA: u = (v[2], v[0], v[1]);   MIC: u_i = fmaf(M[i][2], v[2], fmaf(M[i][1], v[1], M[i][0] v[0]))
//     n = sqrtf(fmaf(u_z, u_z, fmaf(u_y, u_y, u_x u_x)));  no vote unless norm_lo <= n <= norm_hi;  u /= n
//     score[g] = sum over the votes, in vote order, of max(0, (dot(u, U[g]) - c0) inv),  dot = fmaf(u_z, U_z, fmaf(u_y, U_y, u_x U_x))
// and K peaks are picked greedily: the unsuppressed cell of greatest score (lowest index on a tie), stop below min_score, refine to
// m / |m| with m the vote-order sum of the votes with dot(u, U[g*]) >= c0, suppress the cells with dot(U[g], U[g*]) >= cos_suppress.
//
//   doa_hist_kernel<CPT>   one workgroup of 256 threads per (clip, label frame).
//     1. compaction: 256 cells at a time, one per thread (consecutive lanes read consecutive columns); a ballot per wave and the four
//        waves' counts through LDS (two alternating rows, ONE barrier per 256 cells) put the valid votes into LDS in vote order, as three
//        planes x, y, z: at most 4096 votes, 48 KiB.
//     2. scores: thread t owns the cells t, t + 256, ... (CPT of them), their unit vectors and running scores in registers; every
//        thread walks the votes, all lanes reading the same LDS word (a broadcast, no bank conflict).  7 VALU per (vote, cell).
//     3. peaks, K times: best (score, lowest index) of the thread's unsuppressed cells, a 64-lane butterfly, the four waves' winners
//        through LDS (a row per k: nothing is reused), one barrier.  Wave 0 refines: 64 votes test the cap at once, the ballot is walked
//        bit by bit in vote order by scalar code, so the sum costs the votes inside the cap, not all of them.  Meanwhile every thread
//        suppresses its own cells in a register bit mask.
// No atomics, no global scratch, every sum in a fixed order: two calls give equal bits and a clip's result does not depend on its batch.
// A frame without votes skips step 2.  Feature offsets are 64-bit.  LDS 48.2 KiB: three workgroups per CU.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int MAX_VOTES = 4096, MAX_SOURCES = 8, MAX_CPT = 28, MAX_CELLS = MAX_CPT * THREADS;
constexpr int MIN_STEP = 3, MAX_STEP = 30;

struct doa_args {
    const float *feat;
    const float *grid;          // [G][3] unit vectors (x, y, z)
    int *count, *votes, *cell;
    float *score, *direction, *spectrum;
    int64_t T;
    int Cf, F, col0, ncol, P, Fl, G, K, mic;
    float M[9];
    float c0, inv, cos_sup, min_score, norm_lo, norm_hi;
};

__device__ __forceinline__ float dot3(float ux, float uy, float uz, float gx, float gy, float gz)
{
    return fmaf(uz, gz, fmaf(uy, gy, ux * gx));
}

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

template <int CPT>
__global__ __launch_bounds__(THREADS) void doa_hist_kernel(const doa_args a)
{
    __shared__ float vx[MAX_VOTES], vy[MAX_VOTES], vz[MAX_VOTES];
    __shared__ int wave_count[2][WAVES];
    __shared__ float best_s[MAX_SOURCES][WAVES];
    __shared__ int best_g[MAX_SOURCES][WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)(blockIdx.x / (unsigned)a.Fl), f = (int)(blockIdx.x - (unsigned)b * (unsigned)a.Fl);
    const int64_t plane = a.T * a.F;
    const float *p4 = a.feat + ((int64_t)b * a.Cf + 4) * plane + (int64_t)f * a.P * a.F + a.col0;
    const int ncells = a.P * a.ncol;

    // 1. the valid votes into LDS, in vote order
    int n = 0;
    for (int first = 0, round = 0; first < ncells; first += THREADS, round++) {
        const int c = first + tid;
        float ux = 0.f, uy = 0.f, uz = 0.f;
        bool ok = false;
        if (c < ncells) {
            const int t = c / a.ncol, col = c - t * a.ncol;
            const float *q = p4 + (int64_t)t * a.F + col;
            const float v0 = q[0], v1 = q[plane], v2 = q[2 * plane];
            ok = finite_bits(v0) && finite_bits(v1) && finite_bits(v2) && !(v0 == 0.f && v1 == 0.f && v2 == 0.f);
            if (a.mic) {
                ux = fmaf(a.M[2], v2, fmaf(a.M[1], v1, a.M[0] * v0));
                uy = fmaf(a.M[5], v2, fmaf(a.M[4], v1, a.M[3] * v0));
                uz = fmaf(a.M[8], v2, fmaf(a.M[7], v1, a.M[6] * v0));
            } else {
                ux = v2, uy = v0, uz = v1;
            }
            const float len = sqrtf(fmaf(uz, uz, fmaf(uy, uy, ux * ux)));
            ok = ok && len >= a.norm_lo && len <= a.norm_hi;        // (a NaN or infinite length fails both)
            ux /= len, uy /= len, uz /= len;
        }
        const unsigned long long mask = __ballot(ok);
        if (lane == 0) wave_count[round & 1][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const int cw = wave_count[round & 1][w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (ok) {
            const int at = n + before + __popcll(mask & ((1ull << lane) - 1ull));       // < MAX_VOTES: ncells <= MAX_VOTES
            vx[at] = ux, vy[at] = uy, vz[at] = uz;
        }
        n += total;
    }
    __syncthreads();

    // 2. the scores of this thread's cells
    float gx[CPT], gy[CPT], gz[CPT], sc[CPT];
#pragma unroll
    for (int i = 0; i < CPT; i++) {
        const int g = tid + i * THREADS;
        const bool in = g < a.G;
        gx[i] = in ? a.grid[3 * g] : 0.f;
        gy[i] = in ? a.grid[3 * g + 1] : 0.f;
        gz[i] = in ? a.grid[3 * g + 2] : 0.f;
        sc[i] = 0.f;
    }
    const float c0 = a.c0, inv = a.inv;
#pragma unroll 2
    for (int v = 0; v < n; v++) {
        const float ux = vx[v], uy = vy[v], uz = vz[v];
#pragma unroll
        for (int i = 0; i < CPT; i++) sc[i] += fmaxf(0.f, (dot3(ux, uy, uz, gx[i], gy[i], gz[i]) - c0) * inv);
    }
    const int64_t frame = (int64_t)b * a.Fl + f;
    if (a.spectrum) {
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int g = tid + i * THREADS;
            if (g < a.G) a.spectrum[frame * a.G + g] = sc[i];
        }
    }

    // 3. the peaks
    unsigned suppressed = 0;
    int k = 0;
    for (; k < a.K; k++) {
        float s = -1.f;
        int g = INT_MAX;
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int gi = tid + i * THREADS;
            if (gi < a.G && !((suppressed >> i) & 1u) && sc[i] > s) s = sc[i], g = gi;       // ascending gi: the lowest index of a tie stays
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(s, off);
            const int og = __shfl_xor(g, off);
            if (os > s || (os == s && og < g)) s = os, g = og;
        }
        if (lane == 0) best_s[k][wave] = s, best_g[k][wave] = g;
        __syncthreads();
        s = best_s[k][0], g = best_g[k][0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) {
            const float os = best_s[k][w];
            const int og = best_g[k][w];
            if (os > s || (os == s && og < g)) s = os, g = og;
        }
        if (g == INT_MAX || !(s >= a.min_score)) break;             // the same in every thread
        const float px = a.grid[3 * g], py = a.grid[3 * g + 1], pz = a.grid[3 * g + 2];
        if (wave == 0) {
            float mx = 0.f, my = 0.f, mz = 0.f;
            for (int v0 = 0; v0 < n; v0 += 64) {
                const int v = v0 + lane;
                unsigned long long inside = __ballot(v < n && dot3(vx[v < n ? v : 0], vy[v < n ? v : 0], vz[v < n ? v : 0], px, py, pz) >= c0);
                while (inside) {                                    // wave-uniform: the votes inside the cap, in vote order
                    const int j = v0 + __builtin_ctzll(inside);
                    inside &= inside - 1;
                    mx += vx[j], my += vy[j], mz += vz[j];
                }
            }
            if (lane == 0) {
                const float len = sqrtf(fmaf(mz, mz, fmaf(my, my, mx * mx)));
                const int64_t at = frame * a.K + k;
                a.cell[at] = g;
                a.score[at] = s;
                a.direction[3 * at] = mx / len;
                a.direction[3 * at + 1] = my / len;
                a.direction[3 * at + 2] = mz / len;
            }
        }
#pragma unroll
        for (int i = 0; i < CPT; i++)
            if (dot3(gx[i], gy[i], gz[i], px, py, pz) >= a.cos_sup) suppressed |= 1u << i;
    }
    if (wave == 0) {
        if (lane == 0) a.count[frame] = k, a.votes[frame] = n;
        if (lane >= k && lane < a.K) {                              // the unused slots
            const int64_t at = frame * a.K + lane;
            a.cell[at] = -1;
            a.score[at] = 0.f;
            a.direction[3 * at] = 0.f, a.direction[3 * at + 1] = 0.f, a.direction[3 * at + 2] = 0.f;
        }
    }
}

__attribute__((format(printf, 2, 3))) int hfail(int code, const char *fmt, ...)
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

extern "C" int salsa_doa_hist_limits(int *max_votes, int *max_sources, int *max_cells)
{
    if (max_votes) *max_votes = MAX_VOTES;
    if (max_sources) *max_sources = MAX_SOURCES;
    if (max_cells) *max_cells = MAX_CELLS;
    return THREADS;
}

extern "C" int salsa_doa_hist_cells(int grid_step)
{
    if (grid_step < MIN_STEP || grid_step > MAX_STEP || 90 % grid_step) return 0;
    return (360 / grid_step) * (180 / grid_step - 1) + 2;
}

extern "C" int salsa_doa_hist_supported(int n_channels, int n_freq, int col0, int col1, int frames_per_label, int grid_step, int max_sources)
{
    if (n_channels < 7 || n_freq < 1 || col0 < 0 || col1 <= col0 || col1 > n_freq || frames_per_label < 1) return 0;
    if ((int64_t)frames_per_label * (col1 - col0) > MAX_VOTES) return 0;
    if (max_sources < 1 || max_sources > MAX_SOURCES) return 0;
    return salsa_doa_hist_cells(grid_step) ? 1 : 0;
}

extern "C" int salsa_doa_hist(const float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq, int col0, int col1,
                              int frames_per_label, int audio_format, const float *mic_matrix, const float *d_grid, int grid_step,
                              float cos_kernel, float inv_kernel, float cos_suppress, float min_score, float norm_lo, float norm_hi,
                              int max_sources, int *d_count, int *d_votes, int *d_cell, float *d_score, float *d_direction,
                              float *d_spectrum, void *hip_stream)
{
    const char *who = "salsa_doa_hist";
    if (!d_feat || !d_grid || !d_count || !d_votes || !d_cell || !d_score || !d_direction) return hfail(-1, "%s: null pointer", who);
    if (audio_format != SALSA_FORMAT_FOA && audio_format != SALSA_FORMAT_MIC) return hfail(-1, "%s: the format is FOA or MIC", who);
    if (audio_format == SALSA_FORMAT_MIC && !mic_matrix) return hfail(-1, "%s: the MIC format needs its 3 x 3 matrix", who);
    if (!salsa_doa_hist_supported(n_channels, n_freq, col0, col1, frames_per_label, grid_step, max_sources))
        return hfail(-1, "%s: >= 7 channels, 0 <= col0 < col1 <= n_freq, at most %d cells per label frame, a grid step of %d .. %d that "
                         "divides 90, 1 .. %d sources", who, MAX_VOTES, MIN_STEP, MAX_STEP, MAX_SOURCES);
    if (batch < 1 || n_frames < frames_per_label) return hfail(-1, "%s: batch >= 1 and at least one label frame", who);
    const int64_t Fl = n_frames / frames_per_label;
    if (Fl * batch > 0x7fffffffll) return hfail(-1, "%s: more than 2^31 - 1 label frames", who);
    if (!(cos_kernel > -1.f && cos_kernel < 1.f) || !(inv_kernel > 0.f) || !(cos_suppress >= -1.f && cos_suppress <= 0.9999f))
        return hfail(-1, "%s: -1 < cos_kernel < 1, inv_kernel > 0, -1 <= cos_suppress <= 0.9999 (a peak suppresses its own cell)", who);
    if (!(min_score > 0.f) || !(norm_lo > 0.f) || !(norm_hi >= norm_lo) || !(norm_hi <= 3.0e38f))
        return hfail(-1, "%s: min_score > 0 and 0 < norm_lo <= norm_hi, finite", who);
    doa_args a;
    a.feat = d_feat, a.grid = d_grid;
    a.count = d_count, a.votes = d_votes, a.cell = d_cell;
    a.score = d_score, a.direction = d_direction, a.spectrum = d_spectrum;
    a.T = n_frames, a.Cf = n_channels, a.F = n_freq, a.col0 = col0, a.ncol = col1 - col0, a.P = frames_per_label, a.Fl = (int)Fl;
    a.G = salsa_doa_hist_cells(grid_step), a.K = max_sources, a.mic = audio_format == SALSA_FORMAT_MIC;
    for (int i = 0; i < 9; i++) a.M[i] = a.mic ? mic_matrix[i] : 0.f;
    a.c0 = cos_kernel, a.inv = inv_kernel, a.cos_sup = cos_suppress, a.min_score = min_score, a.norm_lo = norm_lo, a.norm_hi = norm_hi;
    const dim3 grid((unsigned)(Fl * batch)), block(THREADS);
    hipStream_t st = (hipStream_t)hip_stream;
    if (a.G <= 4 * THREADS)
        hipLaunchKernelGGL(doa_hist_kernel<4>, grid, block, 0, st, a);
    else if (a.G <= 10 * THREADS)
        hipLaunchKernelGGL(doa_hist_kernel<10>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(doa_hist_kernel<MAX_CPT>, grid, block, 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : hfail(-6, "%s: launch failed", who);
}
