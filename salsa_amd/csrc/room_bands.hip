// room_bands.hip -- the filter sums of shoebox rooms whose walls differ per octave band (include/salsa_hip.h: salsa_band_merge,
// salsa_band_split, salsa_room_max_bands).  A banded room has K amplitude rows A_b over one image table; its response is
// the sum over the bands of the band's image-source response r_b (room_rir.hip: salsa_room_rirs_bands), filtered by the band's linear-phase
// filter h_b (2 D + 1 taps, centre D):
//     h[s, c, k] = sum_b sum_{j = 0}^{2 D} h_b[j] r_b[s, c, k + D - j],   r_b on the taps -D .. L + D - 1.
//
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
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "room_gather.h" // MAX_BANDS, room_fail

namespace {

using namespace room;

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

int check_fir(const char *who, const void *a, const void *b, const void *c, int n, int K, int L, int half)
{
    if (!a || !b || !c) return room_fail(-1, "%s: null pointer", who);
    if (n < 1 || n > FB_MAX_ROWS) return room_fail(-1, "%s: 1 .. %d rows", who, FB_MAX_ROWS);
    if (K < 1 || K > MAX_BANDS) return room_fail(-1, "%s: 1 .. %d bands", who, MAX_BANDS);
    if (L < 1 || L > FB_MAX_LEN) return room_fail(-1, "%s: 1 <= length <= %d", who, FB_MAX_LEN);
    if (half < 1 || half > FB_MAX_HALF) return room_fail(-1, "%s: 1 <= half <= %d", who, FB_MAX_HALF);
    return 0;
}

} // namespace

extern "C" int salsa_room_max_bands(void) { return MAX_BANDS; }

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
    return hipGetLastError() == hipSuccess ? 0 : room_fail(-6, "salsa_band_merge: launch failed");
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
    return hipGetLastError() == hipSuccess ? 0 : room_fail(-6, "salsa_band_split: launch failed");
}
