// room_rir.hip -- shoebox room responses of an open array by the image-source method (include/salsa_hip.h: salsa_room_rirs, salsa_room_rirs_bands,
// salsa_room_max_images, salsa_room_tap_block; DESIGN.md sections 9m and 9p).
// The host has enumerated the room's images once (salsa_amd/rooms.py: room_images): image i mirrors a source s to p_i = sign_i o s +
// shift_i with one amplitude A_i,b per band b (K rows; a room without bands has one).  For a receiver point rho, d = |p - rho|, tau =
// d fs / c - t0, and the image adds
//     g (A_b / d) w(k - tau),   w(x) = sinc(x) (1 + cos(pi x / H)) / 2 for |x| < H = 16, else 0
// to tap k of band b (for FOA times (1, u_y, u_z, u_x), u = (p - rho) / d, on the channels W, Y, Z, X, all four from one distance and delay).
//
//   gather_kernel<FOA, K>   room_gather.h's skeleton with K accumulators per channel.  The float64 geometry of an image and, per tap, the
//                           windowed sinc are computed ONCE; the image's K coefficients g A_b / d (times u_c) go into LDS beside (floor tau,
//                           float32 fraction of tau, sin(pi fraction)), and every thread adds weight x coefficient to its K (x 4 for FOA)
//                           accumulators.  The taps start at first_tap, which may be negative: a tap's bits depend on the table alone,
//                           not on first_tap, n_taps or the block it falls in, since a block only leaves out images that do not reach
//                           it.  An amplitude of 0 adds +-0 to a sum that started at +0.0.  salsa_room_rirs is the <FOA, 1>
//                           instantiation from tap 0: for K = 1 the output layout [source][channel][band][tap] is its own.
//
// Precision split: p, d, tau, floor(tau) and tau - floor(tau) are float64 (at 16384 taps one float32 ulp of tau is 0.002 samples, 0.6 % of
// that image's contribution); the coefficient g A / d (times u_c) is formed in float64 and rounded once.  From the tap argument on
// everything is float32: x = (float)(k - floor tau) - (float)frac (an integer of magnitude <= 16 minus a fraction: no cancellation of a
// large tau), sin(pi x) = -(-1)^j sin(pi frac) by the addition theorem (sinpif once per image, exact zeros at integer delays), the
// window by cospif(x / 16), one IEEE division per tap and image, float32 accumulation.
//
// The LDS holds 256 compacted images x (12 + 4 K NC) bytes -- 7 KiB for one band of FOA, 4 KiB omni, 35 KiB for eight bands of FOA --, so
// with one band LDS never limits residency and the registers do not either (a few dozen: eight waves per SIMD).
// The launchers check everything on the host before the first device call; all output offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "room_gather.h"

namespace {

using namespace room;

constexpr int MAX_LEAD = 4096, MAX_BAND_TAPS = MAX_RIR + MAX_LEAD;   // salsa_room_rirs_bands: |first tap| and the taps of one call

struct gather_args {
    double rec[MAX_RECEIVERS][3];
    double fs_over_c;
    int n_images, first_tap, n_taps;
};

template <bool FOA, int K>
__global__ __launch_bounds__(THREADS) void gather_kernel(const double *__restrict__ images, const double *__restrict__ sources,
                                                         const gather_args a, float *__restrict__ out)
{
    constexpr int NC = FOA ? 4 : 1;
    __shared__ int s_k0[THREADS];
    __shared__ float s_f[THREADS], s_sp[THREADS], s_c[THREADS][K * NC];
    __shared__ int s_count[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = (int)blockIdx.y, r = (int)blockIdx.z;
    const int end = a.first_tap + a.n_taps;
    const int lo = a.first_tap + (int)blockIdx.x * TAPS, hi = min(lo + TAPS, end);   // this block's taps [lo, hi)
    const int k = lo + tid;
    const source_row s = load_source(sources, r);
    const double qx = a.rec[m][0], qy = a.rec[m][1], qz = a.rec[m][2];
    // floor(tau) of an image that reaches the block: its taps floor(tau) - H + 1 .. floor(tau) + H meet [lo, hi)
    const double f_lo = (double)(lo - H), f_hi = (double)(hi + H - 2);
    const int64_t n = a.n_images;
    float acc[K][NC];
#pragma unroll
    for (int b = 0; b < K; b++)
#pragma unroll
        for (int c = 0; c < NC; c++) acc[b][c] = 0.f;

    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + tid;
        bool hit = false;
        int k0 = 0;
        float fr = 0.f, co[K][NC];
#pragma unroll
        for (int b = 0; b < K; b++)
#pragma unroll
            for (int c = 0; c < NC; c++) co[b][c] = 0.f;
        if (i < n) {
            const image_path p = image_geometry(images, n, i, s, qx, qy, qz, a.fs_over_c);
            hit = image_reaches(p.tf, f_lo, f_hi);
            if (hit) {
                k0 = (int)p.tf;
                fr = (float)(p.tau - p.tf);
#pragma unroll
                for (int b = 0; b < K; b++) {
                    const double amp = image_gain(images, n, i, b, s.g, p.d);
                    co[b][0] = (float)amp;
                    if (FOA) {
                        co[b][1] = (float)(amp * (p.dy / p.d));
                        co[b][2] = (float)(amp * (p.dz / p.d));
                        co[b][3] = (float)(amp * (p.dx / p.d));
                    }
                }
            }
        }
        int pos, total;
        compact(hit, s_count, lane, w, pos, total);
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
            if (j < 1 - H || j > H) continue;
            const float x = (float)j - s_f[e];
            if (!(fabsf(x) < (float)H)) continue;
            const float wv = tap_weight(x, j, s_sp[e]);
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

template <bool FOA>
void launch_gather(int K, dim3 grid, hipStream_t s, const double *images, const double *sources, const gather_args &a, float *out)
{
#define ROOM_GATHER_CASE(k) hipLaunchKernelGGL((gather_kernel<FOA, k>), grid, dim3(THREADS), 0, s, images, sources, a, out)
    switch (K) {
    case 1: ROOM_GATHER_CASE(1); break;
    case 2: ROOM_GATHER_CASE(2); break;
    case 3: ROOM_GATHER_CASE(3); break;
    case 4: ROOM_GATHER_CASE(4); break;
    case 5: ROOM_GATHER_CASE(5); break;
    case 6: ROOM_GATHER_CASE(6); break;
    case 7: ROOM_GATHER_CASE(7); break;
    default: ROOM_GATHER_CASE(8); break;
    }
#undef ROOM_GATHER_CASE
}

// both entry points from here on: the mode and the receivers' count, the common checks, the launch.  zero_allowed: an amplitude may be 0.
int run_gather(const char *who, const double *images, const double *images_dev, int n_images, int n_bands, bool zero_allowed,
               const double *sources, const double *sources_dev, int n_sources, const double *receivers, int n_receivers, int mode,
               double fs_over_c, int first_tap, int n_taps, float *out, void *hip_stream)
{
    if (!images || !images_dev || !sources || !sources_dev || !receivers || !out) return room_fail(-1, "%s: null pointer", who);
    if (mode != SALSA_ROOM_OMNI && mode != SALSA_ROOM_FOA) return room_fail(-1, "%s: mode is SALSA_ROOM_OMNI or SALSA_ROOM_FOA", who);
    if (n_receivers < 1 || n_receivers > MAX_RECEIVERS || (mode == SALSA_ROOM_FOA && n_receivers != 1))
        return room_fail(-1, "%s: 1 .. %d receivers, exactly one for FOA", who, MAX_RECEIVERS);
    gather_args a;
    if (int rc = check_common(who, images, n_images, n_bands, zero_allowed, sources, n_sources, fs_over_c, receivers, n_receivers,
                              "a receiver position", &a.rec[0][0], MAX_RECEIVERS))
        return rc;
    a.fs_over_c = fs_over_c;
    a.n_images = n_images;
    a.first_tap = first_tap;
    a.n_taps = n_taps;
    const dim3 grid((unsigned)((n_taps + TAPS - 1) / TAPS), (unsigned)n_receivers, (unsigned)n_sources);
    if (mode == SALSA_ROOM_FOA)
        launch_gather<true>(n_bands, grid, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    else
        launch_gather<false>(n_bands, grid, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    return hipGetLastError() == hipSuccess ? 0 : room_fail(-6, "%s: launch failed", who);
}

} // namespace

extern "C" int salsa_room_max_images(void) { return MAX_IMAGES; }
extern "C" int salsa_room_tap_block(void) { return TAPS; }

// one band from tap 0, and the stricter contract: an image without amplitude does not belong in the table
extern "C" int salsa_room_rirs(const double *images, const double *images_dev, int n_images, const double *sources, const double *sources_dev,
                               int n_sources, const double *receivers, int n_receivers, int mode, double fs_over_c, int rir_len,
                               float *out, void *hip_stream)
{
    if (rir_len < 1 || rir_len > MAX_RIR) return room_fail(-1, "salsa_room_rirs: 1 <= rir length <= %d", MAX_RIR);
    return run_gather("salsa_room_rirs", images, images_dev, n_images, 1, false, sources, sources_dev, n_sources, receivers, n_receivers, mode,
                      fs_over_c, 0, rir_len, out, hip_stream);
}

extern "C" int salsa_room_rirs_bands(const double *images, const double *images_dev, int n_images, int n_bands, const double *sources,
                                     const double *sources_dev, int n_sources, const double *receivers, int n_receivers, int mode,
                                     double fs_over_c, int first_tap, int n_taps, float *out, void *hip_stream)
{
    const char *who = "salsa_room_rirs_bands";
    if (n_bands < 1 || n_bands > MAX_BANDS) return room_fail(-1, "%s: 1 .. %d bands", who, MAX_BANDS);
    if (first_tap < -MAX_LEAD || first_tap > MAX_LEAD) return room_fail(-1, "%s: |first tap| <= %d", who, MAX_LEAD);
    if (n_taps < 1 || n_taps > MAX_BAND_TAPS) return room_fail(-1, "%s: 1 <= taps <= %d", who, MAX_BAND_TAPS);
    return run_gather(who, images, images_dev, n_images, n_bands, true, sources, sources_dev, n_sources, receivers, n_receivers, mode, fs_over_c,
                      first_tap, n_taps, out, hip_stream);
}
