// room_bands.hip -- shoebox rooms whose walls differ per octave band (include/salsa_hip.h: salsa_room_rirs_bands, salsa_band_merge,
// salsa_band_split).  A banded room has K amplitude rows A_b over one image table; its response is the sum over
// the bands of the band's image-source response r_b, filtered by the band's linear-phase filter h_b (2 D + 1 taps, centre D):
//     h[s, c, k] = sum_b sum_{j = 0}^{2 D} h_b[j] r_b[s, c, k + D - j],   r_b on the taps -D .. L + D - 1.
//
//   bands_kernel<FOA, K>   room_rir.hip's GATHER with K accumulators per channel: one workgroup owns RB_TAPS = 256 consecutive taps of
//                          one (source, receiver), one tap per thread, and walks the image table in table order, 256 images at a time.
//                          The float64 geometry of an image -- position, distance, delay, its floor and fraction -- and, per tap, the
//                          windowed sinc are computed ONCE; the image's K coefficients g A_b / d (times u_c), each formed in float64 and
//                          rounded once, go into LDS beside (floor tau, fraction, sin(pi fraction)), compacted in table order, and every
//                          thread adds weight x coefficient to its K (x 4 for FOA) accumulators.  The taps start at first_tap, which may
//                          be negative: a tap's bits depend on the table alone, not on first_tap, n_taps or the block it falls in, since
//                          a block only leaves out images that do not reach it.  With K = 1 and first_tap = 0 this IS room_kernel: the
//                          same expressions in the same order, the same bits.  An amplitude of 0 adds +-0 to a sum that started at +0.0.
//   fir_kernel<MERGE>      the two filter sums, direct form from LDS, float32.  A workgroup owns FB_OUT = 2048 consecutive outputs of one
//                          row, eight consecutive outputs per thread; per band it stages the FB_OUT + 2 D inputs it needs in LDS (zeros
//                          outside the row) and every output runs ONE chain acc = fmaf(h_b[j], x_b[k + 2 D - j], acc), b ascending
//                          outside, j ascending inside, from +0.0.  The filter taps are wave-uniform (scalar loads); the inputs of a
//                          thread's eight outputs over eight taps are a window of 15 values held in registers, eight of them new per
//                          eight taps: one LDS read per eight FMAs.  Lanes read at a stride of eight floats, so the LDS image is padded by
//                          one float per 32 (index p + p / 32): the 32 lanes of a read group then fall on 32 different banks.  The taps
//                          are walked in groups of eight, the last group filled with zero taps, which change no bit of a chain that
//                          started at +0.0 (it is never -0.0).  An impulse in gives the filter's taps bit for bit: every other term is a
//                          signed zero.
// Why the direct form: with D = 1024 an output takes K (2 D + 1) = 14343 FMAs, and a bank of 288 rows x 7200 taps 3 x 10^10 -- about a
// millisecond of the float32 vector rate, the same order as the gather that feeds it -- while its sum order is a plain chain that a
// test can restate.  A partitioned FFT on scene_fft.h would do less arithmetic but fix the bits to that FFT's butterflies; it was not
// built.  The launchers check everything on the host before the first device call; all global offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int RB_THREADS = 256, RB_WAVES = 4, RB_TAPS = 256;   // one tap per thread
constexpr int RB_H = 16;                                       // half width of the Hann-windowed sinc (scenes.SINC_HALF)
constexpr int RB_MAX_BANDS = 8, RB_MAX_LEAD = 4096, RB_MAX_TAPS = 16384 + RB_MAX_LEAD;
constexpr int RB_MAX_IMAGES = 1 << 22, RB_MAX_SOURCES = 65535, RB_MAX_RECEIVERS = 4;
constexpr int RB_SOURCE_COLS = 5;

struct bands_args {
    double rec[RB_MAX_RECEIVERS][3];
    double fs_over_c;
    int n_images, first_tap, n_taps;
};

// w(x) for |x| < H of the tap j = k - floor(tau), x = j - frac, given sp = sin(pi frac): sin(pi x) = -(-1)^j sp (room_rir.hip's)
__device__ inline float band_tap_weight(float x, int j, float sp)
{
    if (x == 0.f) return 1.f;
    const float s = (j & 1) ? sp : -sp;
    return s / (3.14159265358979323846f * x) * (0.5f * (1.f + cospif(x * (1.f / RB_H))));
}

template <bool FOA, int K>
__global__ __launch_bounds__(RB_THREADS) void bands_kernel(const double *__restrict__ images, const double *__restrict__ sources,
                                                           const bands_args a, float *__restrict__ out)
{
    constexpr int NC = FOA ? 4 : 1;
    __shared__ int s_k0[RB_THREADS];
    __shared__ float s_f[RB_THREADS], s_sp[RB_THREADS], s_c[RB_THREADS][K * NC];
    __shared__ int s_count[RB_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = (int)blockIdx.y, r = (int)blockIdx.z;
    const int end = a.first_tap + a.n_taps;
    const int lo = a.first_tap + (int)blockIdx.x * RB_TAPS, hi = min(lo + RB_TAPS, end);   // this block's taps [lo, hi)
    const int k = lo + tid;
    const double *src = sources + (int64_t)RB_SOURCE_COLS * r;
    const double sx = src[0], sy = src[1], sz = src[2], t0 = src[3], g = src[4];
    const double qx = a.rec[m][0], qy = a.rec[m][1], qz = a.rec[m][2];
    // floor(tau) of an image that reaches the block: its taps floor(tau) - H + 1 .. floor(tau) + H meet [lo, hi)
    const double f_lo = (double)(lo - RB_H), f_hi = (double)(hi + RB_H - 2);
    const int64_t n = a.n_images;
    float acc[K][NC];
#pragma unroll
    for (int b = 0; b < K; b++)
#pragma unroll
        for (int c = 0; c < NC; c++) acc[b][c] = 0.f;

    for (int64_t base = 0; base < n; base += RB_THREADS) {
        const int64_t i = base + tid;
        bool hit = false;
        int k0 = 0;
        float fr = 0.f, co[K][NC];
#pragma unroll
        for (int b = 0; b < K; b++)
#pragma unroll
            for (int c = 0; c < NC; c++) co[b][c] = 0.f;
        if (i < n) {
            const double dx = images[i] * sx + images[3 * n + i] - qx;
            const double dy = images[n + i] * sy + images[4 * n + i] - qy;
            const double dz = images[2 * n + i] * sz + images[5 * n + i] - qz;
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const double tau = d * a.fs_over_c - t0;
            const double tf = floor(tau);
            hit = tf >= f_lo && tf <= f_hi;               // (false for a NaN; bounds tf before it becomes an int)
            if (hit) {
                k0 = (int)tf;
                fr = (float)(tau - tf);
#pragma unroll
                for (int b = 0; b < K; b++) {
                    const double amp = g * images[(6 + b) * n + i] / d;
                    co[b][0] = (float)amp;
                    if (FOA) {
                        co[b][1] = (float)(amp * (dy / d));
                        co[b][2] = (float)(amp * (dz / d));
                        co[b][3] = (float)(amp * (dx / d));
                    }
                }
            }
        }
        // compaction in table order: the lanes before me in my wave, then the waves before mine
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_count[w] = __popcll(mask);
        __syncthreads();
        int pos = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < RB_WAVES; v++) {
            const int cv = s_count[v];
            pos += v < w ? cv : 0;
            total += cv;
        }
        if (hit) {
            s_k0[pos] = k0;
            s_f[pos] = fr;
            s_sp[pos] = sinpif(fr);
#pragma unroll
            for (int b = 0; b < K; b++)
#pragma unroll
                for (int c = 0; c < NC; c++) s_c[pos][b * NC + c] = co[b][c];
        }
        __syncthreads();
        for (int e = 0; e < total; e++) {
            const int j = k - s_k0[e];
            if (j < 1 - RB_H || j > RB_H) continue;
            const float x = (float)j - s_f[e];
            if (!(fabsf(x) < (float)RB_H)) continue;
            const float wv = band_tap_weight(x, j, s_sp[e]);
#pragma unroll
            for (int b = 0; b < K; b++)
#pragma unroll
                for (int c = 0; c < NC; c++) acc[b][c] += s_c[e][b * NC + c] * wv;
        }
        __syncthreads();                                  // the entries and the counts are free for the next chunk
    }
    if (k >= hi) return;
    const int64_t t = k - a.first_tap;
#pragma unroll
    for (int b = 0; b < K; b++) {
        if (FOA) {
#pragma unroll
            for (int c = 0; c < NC; c++) out[(((int64_t)r * 4 + c) * K + b) * a.n_taps + t] = acc[b][c];
        } else {
            out[(((int64_t)r * gridDim.y + m) * K + b) * a.n_taps + t] = acc[b][0];
        }
    }
}

// ---- the filter sums ------------------------------------------------------------------------------------------------------------------
constexpr int FB_THREADS = 256, FB_PER = 8, FB_OUT = FB_THREADS * FB_PER;   // 2048 outputs of one row per workgroup
constexpr int FB_MAX_HALF = 2048, FB_MAX_LEN = 16384, FB_MAX_ROWS = 1 << 20;
constexpr int FB_LEAD = 16;                                                 // LDS slots below the block's first input: the last tap group's reach
constexpr int FB_SLOTS = FB_LEAD + FB_OUT + 2 * FB_MAX_HALF;                // slot q holds input e = block start + q - FB_LEAD
constexpr int FB_LDS = FB_SLOTS + FB_SLOTS / 32 + 1;

__device__ __forceinline__ int fb_pad(int p) { return p + (p >> 5); }

// MERGE: src [n][K][L + 2 half], out [n][L], the bands summed into one chain.  Split: src [n][L], out [n][K][L], band = blockIdx.z, and
// input e of the extended row is src[e - half], zero outside [0, L).
template <bool MERGE>
__global__ __launch_bounds__(FB_THREADS) void fir_kernel(const float *__restrict__ src, const float *__restrict__ filters, int K, int L,
                                                         int half, float *__restrict__ out)
{
    __shared__ float s_x[FB_LDS];
    const int tid = (int)threadIdx.x;
    const int row = (int)blockIdx.y;
    const int kb = (int)blockIdx.x * FB_OUT;                                  // the block's outputs [kb, kb + FB_OUT) below L
    const int n_taps = 2 * half + 1, n_ext = L + 2 * half;
    const int n_groups = (n_taps + 7) / 8;
    const int slots = FB_LEAD + FB_OUT + 2 * half;
    const int q0 = FB_LEAD + FB_PER * tid;                                    // the slot of input e = k0 = kb + 8 tid
    float acc[FB_PER];
#pragma unroll
    for (int i = 0; i < FB_PER; i++) acc[i] = 0.f;

    const int b_lo = MERGE ? 0 : (int)blockIdx.z, b_hi = MERGE ? K : b_lo + 1;
    for (int b = b_lo; b < b_hi; b++) {
        if (MERGE && b > b_lo) __syncthreads();                               // the last band's reads are done
        const float *x = MERGE ? src + ((int64_t)row * K + b) * n_ext : src + (int64_t)row * L;
        for (int q = tid; q < slots; q += FB_THREADS) {
            const int e = kb + q - FB_LEAD;                                   // index into the extended row
            float v = 0.f;
            if (MERGE) {
                if (e >= 0 && e < n_ext) v = x[e];
            } else {
                if (e >= half && e < half + L) v = x[e - half];
            }
            s_x[fb_pad(q)] = v;
        }
        __syncthreads();
        const float *hf = filters + (int64_t)b * n_taps;
        // output i of this thread at tap j reads slot q0 + i + 2 half - j; hi_[.] = slots P .. P + 7, lo_[.] = P - 8 .. P - 1, P = q0 + 2 half - j0
        float hi_[8], lo_[8];
        int P = q0 + 2 * half;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            hi_[u] = s_x[fb_pad(P + u)];
            lo_[u] = s_x[fb_pad(P - 8 + u)];
        }
        for (int gidx = 0; gidx < n_groups; gidx++) {
            const int j0 = 8 * gidx;
            float hv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int j = j0 + u;
                const float t = hf[min(j, n_taps - 1)];
                hv[u] = j < n_taps ? t : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
#pragma unroll
                for (int i = 0; i < FB_PER; i++) {
                    const int mm = 8 - u + i;                                 // 1 .. 15: the slot P - 8 + mm
                    acc[i] = __builtin_fmaf(hv[u], mm < 8 ? lo_[mm] : hi_[mm - 8], acc[i]);
                }
            P -= 8;
#pragma unroll
            for (int u = 0; u < 8; u++) hi_[u] = lo_[u];
            if (gidx + 1 < n_groups) {
#pragma unroll
                for (int u = 0; u < 8; u++) lo_[u] = s_x[fb_pad(P - 8 + u)];
            }
        }
        if (!MERGE) break;
    }
    const int k0 = kb + FB_PER * tid;
    float *o = MERGE ? out + (int64_t)row * L : out + ((int64_t)row * K + b_lo) * L;
#pragma unroll
    for (int i = 0; i < FB_PER; i++)
        if (k0 + i < L) o[k0 + i] = acc[i];
}

__attribute__((format(printf, 2, 3))) int bfail(int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    salsa_set_last_error_(msg);
    return code;
}

template <bool FOA, int K>
void launch_bands(dim3 grid, hipStream_t s, const double *images, const double *sources, const bands_args &a, float *out)
{
    hipLaunchKernelGGL((bands_kernel<FOA, K>), grid, dim3(RB_THREADS), 0, s, images, sources, a, out);
}

template <bool FOA>
void launch_bands_k(int K, dim3 grid, hipStream_t s, const double *images, const double *sources, const bands_args &a, float *out)
{
    switch (K) {
    case 1: launch_bands<FOA, 1>(grid, s, images, sources, a, out); break;
    case 2: launch_bands<FOA, 2>(grid, s, images, sources, a, out); break;
    case 3: launch_bands<FOA, 3>(grid, s, images, sources, a, out); break;
    case 4: launch_bands<FOA, 4>(grid, s, images, sources, a, out); break;
    case 5: launch_bands<FOA, 5>(grid, s, images, sources, a, out); break;
    case 6: launch_bands<FOA, 6>(grid, s, images, sources, a, out); break;
    case 7: launch_bands<FOA, 7>(grid, s, images, sources, a, out); break;
    default: launch_bands<FOA, 8>(grid, s, images, sources, a, out); break;
    }
}

int check_fir(const char *who, const void *a, const void *b, const void *c, int n, int K, int L, int half)
{
    if (!a || !b || !c) return bfail(-1, "%s: null pointer", who);
    if (n < 1 || n > FB_MAX_ROWS) return bfail(-1, "%s: 1 .. %d rows", who, FB_MAX_ROWS);
    if (K < 1 || K > RB_MAX_BANDS) return bfail(-1, "%s: 1 .. %d bands", who, RB_MAX_BANDS);
    if (L < 1 || L > FB_MAX_LEN) return bfail(-1, "%s: 1 <= length <= %d", who, FB_MAX_LEN);
    if (half < 1 || half > FB_MAX_HALF) return bfail(-1, "%s: 1 <= half <= %d", who, FB_MAX_HALF);
    return 0;
}

} // namespace

extern "C" int salsa_room_max_bands(void) { return RB_MAX_BANDS; }

extern "C" int salsa_room_rirs_bands(const double *images, const double *images_dev, int n_images, int n_bands, const double *sources,
                                     const double *sources_dev, int n_sources, const double *receivers, int n_receivers, int mode,
                                     double fs_over_c, int first_tap, int n_taps, float *out, void *hip_stream)
{
    const char *who = "salsa_room_rirs_bands";
    if (!images || !images_dev || !sources || !sources_dev || !receivers || !out) return bfail(-1, "%s: null pointer", who);
    if (mode != SALSA_ROOM_OMNI && mode != SALSA_ROOM_FOA) return bfail(-1, "%s: mode is SALSA_ROOM_OMNI or SALSA_ROOM_FOA", who);
    if (n_receivers < 1 || n_receivers > RB_MAX_RECEIVERS || (mode == SALSA_ROOM_FOA && n_receivers != 1))
        return bfail(-1, "%s: 1 .. %d receivers, exactly one for FOA", who, RB_MAX_RECEIVERS);
    if (n_bands < 1 || n_bands > RB_MAX_BANDS) return bfail(-1, "%s: 1 .. %d bands", who, RB_MAX_BANDS);
    if (n_images < 1 || n_images > RB_MAX_IMAGES) return bfail(-1, "%s: 1 .. %d images", who, RB_MAX_IMAGES);
    if (n_sources < 1 || n_sources > RB_MAX_SOURCES) return bfail(-1, "%s: 1 .. %d sources", who, RB_MAX_SOURCES);
    if (first_tap < -RB_MAX_LEAD || first_tap > RB_MAX_LEAD) return bfail(-1, "%s: |first tap| <= %d", who, RB_MAX_LEAD);
    if (n_taps < 1 || n_taps > RB_MAX_TAPS) return bfail(-1, "%s: 1 <= taps <= %d", who, RB_MAX_TAPS);
    if (!(fs_over_c > 0.0 && fs_over_c <= 1e9)) return bfail(-1, "%s: fs / c must be positive and finite", who);
    const int64_t n = n_images;
    for (int64_t i = 0; i < n; i++) {
        for (int ax = 0; ax < 3; ax++)
            if (fabs(images[ax * n + i]) != 1.0 || !(fabs(images[(3 + ax) * n + i]) <= 1e9))
                return bfail(-1, "%s: an image's sign is not +-1 or its shift is not finite", who);
        for (int b = 0; b < n_bands; b++)
            if (!(images[(6 + b) * n + i] >= 0.0 && images[(6 + b) * n + i] <= 1.0))
                return bfail(-1, "%s: an image's amplitude is outside [0, 1]", who);
    }
    for (int r = 0; r < n_sources; r++) {
        const double *s = sources + (int64_t)RB_SOURCE_COLS * r;
        if (!(fabs(s[0]) <= 1e9 && fabs(s[1]) <= 1e9 && fabs(s[2]) <= 1e9)) return bfail(-1, "%s: a source position is not finite", who);
        if (!(s[3] >= 0.0 && s[3] <= 1e9 && s[3] == floor(s[3]))) return bfail(-1, "%s: a time origin is not a whole number >= 0", who);
        if (!(s[4] > 0.0 && s[4] <= 1e9)) return bfail(-1, "%s: a gain is not positive and finite", who);
    }
    bands_args a;
    for (int m = 0; m < RB_MAX_RECEIVERS; m++)
        for (int ax = 0; ax < 3; ax++) {
            a.rec[m][ax] = m < n_receivers ? receivers[3 * m + ax] : 0.0;
            if (!(fabs(a.rec[m][ax]) <= 1e9)) return bfail(-1, "%s: a receiver position is not finite", who);
        }
    a.fs_over_c = fs_over_c;
    a.n_images = n_images;
    a.first_tap = first_tap;
    a.n_taps = n_taps;
    const dim3 grid((unsigned)((n_taps + RB_TAPS - 1) / RB_TAPS), (unsigned)n_receivers, (unsigned)n_sources);
    if (mode == SALSA_ROOM_FOA)
        launch_bands_k<true>(n_bands, grid, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    else
        launch_bands_k<false>(n_bands, grid, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    return hipGetLastError() == hipSuccess ? 0 : bfail(-6, "%s: launch failed", who);
}

extern "C" int salsa_band_merge(const float *bands, const float *filters, int n, int n_bands, int length, int half, float *out,
                                void *hip_stream)
{
    if (int rc = check_fir("salsa_band_merge", bands, filters, out, n, n_bands, length, half)) return rc;
    for (int y0 = 0; y0 < n; y0 += 65535) {                                   // (grid.y is a 16-bit count)
        const int rows = n - y0 < 65535 ? n - y0 : 65535;
        const dim3 grid((unsigned)((length + FB_OUT - 1) / FB_OUT), (unsigned)rows);
        hipLaunchKernelGGL(fir_kernel<true>, grid, dim3(FB_THREADS), 0, (hipStream_t)hip_stream,
                           bands + (int64_t)y0 * n_bands * (length + 2 * half), filters, n_bands, length, half, out + (int64_t)y0 * length);
    }
    return hipGetLastError() == hipSuccess ? 0 : bfail(-6, "salsa_band_merge: launch failed");
}

extern "C" int salsa_band_split(const float *x, const float *filters, int n, int n_bands, int length, int half, float *out, void *hip_stream)
{
    if (int rc = check_fir("salsa_band_split", x, filters, out, n, n_bands, length, half)) return rc;
    for (int y0 = 0; y0 < n; y0 += 65535) {
        const int rows = n - y0 < 65535 ? n - y0 : 65535;
        const dim3 grid((unsigned)((length + FB_OUT - 1) / FB_OUT), (unsigned)rows, (unsigned)n_bands);
        hipLaunchKernelGGL(fir_kernel<false>, grid, dim3(FB_THREADS), 0, (hipStream_t)hip_stream, x + (int64_t)y0 * length, filters, n_bands,
                           length, half, out + (int64_t)y0 * n_bands * length);
    }
    return hipGetLastError() == hipSuccess ? 0 : bfail(-6, "salsa_band_split: launch failed");
}
