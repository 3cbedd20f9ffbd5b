// room_rir.hip -- shoebox room responses by the image-source method (include/salsa_hip.h: salsa_room_*).
// The host has enumerated the room's images once (salsa_amd/rooms.py: room_images): image i mirrors a source s to p_i = sign_i o s +
// shift_i with the amplitude A_i.  For a receiver point rho, d = |p - rho|, tau = d fs / c - t0, and the image adds
//     g (A / d) w(k - tau),   w(x) = sinc(x) (1 + cos(pi x / H)) / 2 for |x| < H = 16, else 0
// to tap k (for FOA times (1, u_y, u_z, u_x), u = (p - rho) / d, on the channels W, Y, Z, X, all four from one distance and delay).
//
//   room_kernel<FOA>   a GATHER: one workgroup owns RM_TAPS = 256 consecutive taps of one (source, receiver), one tap per thread.  It
//                      walks the image table in table order, 256 images at a time, one per thread: position, distance and delay in
//                      float64; an image whose support (tau - H, tau + H) meets the block is kept.  The kept images are compacted into
//                      LDS IN TABLE ORDER (ballot and popcount inside a wave of 64, the waves' counts summed in wave order), as (floor
//                      tau, float32 fraction of tau, sin(pi fraction), float32 coefficients).  Then every thread adds the kept images to
//                      its own tap, in that order, in float32.  So a tap's sum runs over the images in table order whatever the batch, the
//                      grid or the block are: no atomics, nothing summed across threads, two runs and a source alone or in a batch agree
//                      bit for bit.  A tap no support reaches keeps its initial +0.0f.
//
// Precision split: p, d, tau, floor(tau) and tau - floor(tau) are float64 (at 16384 taps one float32 ulp of tau is 0.002 samples, 0.6 % of
// that image's contribution); the coefficient g A / d (times u_c) is formed in float64 and rounded once.  From the tap argument on
// everything is float32: x = (float)(k - floor tau) - (float)frac (an integer of magnitude <= 16 minus a fraction: no cancellation of a
// large tau), sin(pi x) = -(-1)^j sin(pi frac) by the addition theorem (sinpif once per image, exact zeros at integer delays), the
// window by cospif(x / 16), one IEEE division per tap and image, float32 accumulation.
//
// Block size.  256 threads = 256 taps: four waves fill the four SIMDs of a CU; the LDS holds 256 compacted images x 28 bytes = 7 KiB
// (FOA; 4 KiB omni), so LDS never limits residency and the registers do not either (a few dozen: eight waves per SIMD).  A wider tap block
// would cut the float64 geometry, which every workgroup of a (source, receiver) repeats for the whole table (ceil(len / 256) times
// per image: 29 at 7200 taps), but a block meets images in proportion to its width + 2 H, so at 256 taps the 32 taps of overhang cost
// 12 % and a 7200-tap FOA bank of 72 directions is 2088 workgroups, eight per CU -- enough to hide the barriers of the compaction
// behind other workgroups.  The compacted entries are read by every lane at ONE address (an LDS broadcast, no bank conflict).
// The launcher checks everything on the host before the first device call; all output offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int RM_THREADS = 256, RM_WAVES = 4, RM_TAPS = 256;   // one tap per thread
constexpr int RM_H = 16;                                       // half width of the Hann-windowed sinc (scenes.SINC_HALF)
constexpr int RM_MAX_RIR = 16384, RM_MAX_IMAGES = 1 << 22, RM_MAX_SOURCES = 65535, RM_MAX_RECEIVERS = 4;
constexpr int RM_IMAGE_ROWS = 7, RM_SOURCE_COLS = 5;

struct room_args {
    double rec[RM_MAX_RECEIVERS][3];
    double fs_over_c;
    int n_images, rir_len;
};

// w(x) for |x| < H of the tap j = k - floor(tau), x = j - frac, given sp = sin(pi frac): sin(pi x) = -(-1)^j sp
__device__ inline float tap_weight(float x, int j, float sp)
{
    if (x == 0.f) return 1.f;
    const float s = (j & 1) ? sp : -sp;
    return s / (3.14159265358979323846f * x) * (0.5f * (1.f + cospif(x * (1.f / RM_H))));
}

template <bool FOA>
__global__ __launch_bounds__(RM_THREADS) void room_kernel(const double *__restrict__ images, const double *__restrict__ sources,
                                                          const room_args a, float *__restrict__ out)
{
    constexpr int NC = FOA ? 4 : 1;
    __shared__ int s_k0[RM_THREADS];
    __shared__ float s_f[RM_THREADS], s_sp[RM_THREADS], s_c[RM_THREADS][NC];
    __shared__ int s_count[RM_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = (int)blockIdx.y, r = (int)blockIdx.z;
    const int lo = (int)blockIdx.x * RM_TAPS, hi = min(lo + RM_TAPS, a.rir_len);   // this block's taps [lo, hi)
    const int k = lo + tid;
    const double *src = sources + (int64_t)RM_SOURCE_COLS * r;
    const double sx = src[0], sy = src[1], sz = src[2], t0 = src[3], g = src[4];
    const double qx = a.rec[m][0], qy = a.rec[m][1], qz = a.rec[m][2];
    // floor(tau) of an image that reaches the block: its taps floor(tau) - H + 1 .. floor(tau) + H meet [lo, hi)
    const double f_lo = (double)(lo - RM_H), f_hi = (double)(hi + RM_H - 2);
    const int64_t n = a.n_images;
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0.f;

    for (int64_t base = 0; base < n; base += RM_THREADS) {
        const int64_t i = base + tid;
        bool hit = false;
        int k0 = 0;
        float fr = 0.f, co[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) co[c] = 0.f;
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
                const double amp = g * images[6 * n + i] / d;
                co[0] = (float)amp;
                if (FOA) {
                    co[1] = (float)(amp * (dy / d));
                    co[2] = (float)(amp * (dz / d));
                    co[3] = (float)(amp * (dx / d));
                }
            }
        }
        // compaction in table order: the lanes before me in my wave, then the waves before mine
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_count[w] = __popcll(mask);
        __syncthreads();
        int pos = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < RM_WAVES; v++) {
            const int cv = s_count[v];
            pos += v < w ? cv : 0;
            total += cv;
        }
        if (hit) {
            s_k0[pos] = k0;
            s_f[pos] = fr;
            s_sp[pos] = sinpif(fr);
#pragma unroll
            for (int c = 0; c < NC; c++) s_c[pos][c] = co[c];
        }
        __syncthreads();
        for (int e = 0; e < total; e++) {
            const int j = k - s_k0[e];
            if (j < 1 - RM_H || j > RM_H) continue;
            const float x = (float)j - s_f[e];
            if (!(fabsf(x) < (float)RM_H)) continue;
            const float wv = tap_weight(x, j, s_sp[e]);
#pragma unroll
            for (int c = 0; c < NC; c++) acc[c] += s_c[e][c] * wv;
        }
        __syncthreads();                                  // the entries and the counts are free for the next chunk
    }
    if (k >= hi) return;
    if (FOA) {
#pragma unroll
        for (int c = 0; c < NC; c++) out[((int64_t)r * 4 + c) * a.rir_len + k] = acc[c];
    } else {
        out[((int64_t)r * gridDim.y + m) * a.rir_len + k] = acc[0];
    }
}

__attribute__((format(printf, 2, 3))) int rfail(int code, const char *fmt, ...)
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

extern "C" int salsa_room_max_images(void) { return RM_MAX_IMAGES; }
extern "C" int salsa_room_tap_block(void) { return RM_TAPS; }

extern "C" int salsa_room_rirs(const double *images, const double *images_dev, int n_images, const double *sources, const double *sources_dev,
                               int n_sources, const double *receivers, int n_receivers, int mode, double fs_over_c, int rir_len,
                               float *out, void *hip_stream)
{
    if (!images || !images_dev || !sources || !sources_dev || !receivers || !out) return rfail(-1, "salsa_room_rirs: null pointer");
    if (mode != SALSA_ROOM_OMNI && mode != SALSA_ROOM_FOA) return rfail(-1, "salsa_room_rirs: mode is SALSA_ROOM_OMNI or SALSA_ROOM_FOA");
    if (n_receivers < 1 || n_receivers > RM_MAX_RECEIVERS || (mode == SALSA_ROOM_FOA && n_receivers != 1))
        return rfail(-1, "salsa_room_rirs: 1 .. %d receivers, exactly one for FOA", RM_MAX_RECEIVERS);
    if (n_images < 1 || n_images > RM_MAX_IMAGES) return rfail(-1, "salsa_room_rirs: 1 .. %d images", RM_MAX_IMAGES);
    if (n_sources < 1 || n_sources > RM_MAX_SOURCES) return rfail(-1, "salsa_room_rirs: 1 .. %d sources", RM_MAX_SOURCES);
    if (rir_len < 1 || rir_len > RM_MAX_RIR) return rfail(-1, "salsa_room_rirs: 1 <= rir length <= %d", RM_MAX_RIR);
    if (!(fs_over_c > 0.0 && fs_over_c <= 1e9)) return rfail(-1, "salsa_room_rirs: fs / c must be positive and finite");
    const int64_t n = n_images;
    for (int64_t i = 0; i < n; i++) {
        for (int ax = 0; ax < 3; ax++)
            if (fabs(images[ax * n + i]) != 1.0 || !(fabs(images[(3 + ax) * n + i]) <= 1e9))
                return rfail(-1, "salsa_room_rirs: an image's sign is not +-1 or its shift is not finite");
        if (!(images[6 * n + i] > 0.0 && images[6 * n + i] <= 1.0)) return rfail(-1, "salsa_room_rirs: an image's amplitude is outside (0, 1]");
    }
    for (int r = 0; r < n_sources; r++) {
        const double *s = sources + (int64_t)RM_SOURCE_COLS * r;
        if (!(fabs(s[0]) <= 1e9 && fabs(s[1]) <= 1e9 && fabs(s[2]) <= 1e9)) return rfail(-1, "salsa_room_rirs: a source position is not finite");
        if (!(s[3] >= 0.0 && s[3] <= 1e9 && s[3] == floor(s[3]))) return rfail(-1, "salsa_room_rirs: a time origin is not a whole number >= 0");
        if (!(s[4] > 0.0 && s[4] <= 1e9)) return rfail(-1, "salsa_room_rirs: a gain is not positive and finite");
    }
    room_args a;
    for (int m = 0; m < RM_MAX_RECEIVERS; m++)
        for (int ax = 0; ax < 3; ax++) {
            a.rec[m][ax] = m < n_receivers ? receivers[3 * m + ax] : 0.0;
            if (!(fabs(a.rec[m][ax]) <= 1e9)) return rfail(-1, "salsa_room_rirs: a receiver position is not finite");
        }
    a.fs_over_c = fs_over_c;
    a.n_images = n_images;
    a.rir_len = rir_len;
    const dim3 grid((unsigned)((rir_len + RM_TAPS - 1) / RM_TAPS), (unsigned)n_receivers, (unsigned)n_sources);
    if (mode == SALSA_ROOM_FOA)
        hipLaunchKernelGGL(room_kernel<true>, grid, dim3(RM_THREADS), 0, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    else
        hipLaunchKernelGGL(room_kernel<false>, grid, dim3(RM_THREADS), 0, (hipStream_t)hip_stream, images_dev, sources_dev, a, out);
    return hipGetLastError() == hipSuccess ? 0 : rfail(-6, "salsa_room_rirs: launch failed");
}
