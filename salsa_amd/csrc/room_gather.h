// room_gather.h -- what the image-source room gathers share (room_rir.hip: the open array, broadband and banded; room_sphere.hip: the
// capsules on a rigid sphere; room_bands.hip takes the limits and room_fail).  Included by the room_*.hip units only.
//
// Every gather has the same skeleton.  One workgroup owns TAPS = 256 consecutive taps of one source (and, for the open array, one
// receiver), one tap per thread, and walks the image table IN TABLE ORDER, 256 images at a time, one per thread:
//     image_geometry   position, distance and delay of the image in float64, and floor(tau);
//     image_reaches    an image whose support meets the block's taps is kept;
//     compact          the kept images get consecutive LDS slots in table order (ballot and popcount inside a wave of 64, the waves'
//                      counts summed in wave order), the kernel writes its own entry layout to slot `pos`;
//     barrier; every thread adds the `total` kept images to its own tap, in slot order, in float32; barrier (the entries and the counts
//     are free for the next chunk).
// So a tap's sum runs over the images in table order whatever the batch, the grid or the block are: no atomics, nothing summed across
// threads, two runs and a source alone or in a batch agree bit for bit, and a tap no support reaches keeps its initial +0.0f.  The
// project's bit-level promises for the rooms rest on compact() and on the ONE spelling of the float64 expressions below: the kernels
// differ only in what an LDS entry holds and in how a tap weighs it.
//
// Block size.  256 threads = 256 taps: four waves fill the four SIMDs of a CU.  A wider tap block would cut the float64 geometry, which
// every workgroup of a (source, receiver) repeats for the whole table (ceil(len / 256) times per image: 29 at 7200 taps), but a block
// meets images in proportion to its width + 2 H, so at 256 taps the 32 taps of overhang cost 12 % and a 7200-tap FOA bank of 72
// directions is 2088 workgroups, eight per CU -- enough to hide the barriers of the compaction behind other workgroups.  The compacted
// entries are read by every lane at ONE address (an LDS broadcast, no bank conflict).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace room {

constexpr int THREADS = 256, WAVES = 4, TAPS = 256;   // one tap per thread (salsa_room_tap_block())
constexpr int H = 16;                                 // half width of the Hann-windowed sinc (scenes.SINC_HALF)
constexpr int MAX_RIR = 16384, MAX_IMAGES = 1 << 22, MAX_SOURCES = 65535, MAX_RECEIVERS = 4, MAX_BANDS = 8;
constexpr int IMAGE_ROWS = 6, SOURCE_COLS = 5;        // sign x, y, z, shift x, y, z (the amplitude rows follow); x, y, z, t0, g

// ---- device ---------------------------------------------------------------------------------------------------------------------------
struct source_row { double x, y, z, t0, g; };
struct image_path { double dx, dy, dz, d, tau, tf; };   // image - point, its length, the delay in taps after t0, floor(delay)

__device__ __forceinline__ source_row load_source(const double *__restrict__ sources, int r)
{
    const double *src = sources + (int64_t)SOURCE_COLS * r;
    return {src[0], src[1], src[2], src[3], src[4]};
}

// image i of the n of the table, seen from the point q (a receiver, or the centre of the sphere)
__device__ __forceinline__ image_path image_geometry(const double *__restrict__ images, int64_t n, int64_t i, const source_row &s, double qx,
                                                     double qy, double qz, double fs_over_c)
{
    image_path p;
    p.dx = images[i] * s.x + images[3 * n + i] - qx;
    p.dy = images[n + i] * s.y + images[4 * n + i] - qy;
    p.dz = images[2 * n + i] * s.z + images[5 * n + i] - qz;
    p.d = sqrt(p.dx * p.dx + p.dy * p.dy + p.dz * p.dz);
    p.tau = p.d * fs_over_c - s.t0;
    p.tf = floor(p.tau);
    return p;
}

// floor(tau) of an image that reaches the block lies in [f_lo, f_hi] (false for a NaN; bounds tf before it becomes an int)
__device__ __forceinline__ bool image_reaches(double tf, double f_lo, double f_hi) { return tf >= f_lo && tf <= f_hi; }

// g A_b / d of amplitude row b, in float64; the caller rounds it (times a direction cosine) once
__device__ __forceinline__ double image_gain(const double *__restrict__ images, int64_t n, int64_t i, int b, double g, double d)
{
    return g * images[(IMAGE_ROWS + b) * n + i] / d;
}

// compaction in table order: the lanes before me in my wave, then the waves before mine (lane = tid & 63, w = tid >> 6).  Every thread of
// the block calls it; it holds ONE barrier, the caller another after it has written its entry to slot pos, and a third before the next
// call frees s_count again.
__device__ __forceinline__ void compact(bool hit, int *s_count, int lane, int w, int &pos, int &total)
{
    const unsigned long long mask = __ballot(hit);
    if (lane == 0) s_count[w] = __popcll(mask);
    __syncthreads();
    pos = __popcll(mask & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int v = 0; v < WAVES; v++) {
        const int cv = s_count[v];
        pos += v < w ? cv : 0;
        total += cv;
    }
}

// w(x) for |x| < H of the tap j = k - floor(tau), x = j - frac, given sp = sin(pi frac): sin(pi x) = -(-1)^j sp
__device__ __forceinline__ float tap_weight(float x, int j, float sp)
{
    if (x == 0.f) return 1.f;
    const float s = (j & 1) ? sp : -sp;
    return s / (3.14159265358979323846f * x) * (0.5f * (1.f + cospif(x * (1.f / H))));
}

// ---- host: every launcher checks all it is given before the first device call ---------------------------------------------------------
__attribute__((format(printf, 2, 3))) inline int room_fail(int code, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    salsa_set_last_error_(msg);
    return code;
}

// the host copy of the table: signs +-1, finite shifts, n_amp_rows amplitude rows in (0, 1], or in [0, 1] where a band may carry nothing
inline int check_image_table(const char *who, const double *images, int n_images, int n_amp_rows, bool zero_allowed)
{
    const int64_t n = n_images;
    for (int64_t i = 0; i < n; i++) {
        for (int ax = 0; ax < 3; ax++)
            if (fabs(images[ax * n + i]) != 1.0 || !(fabs(images[(3 + ax) * n + i]) <= 1e9))
                return room_fail(-1, "%s: an image's sign is not +-1 or its shift is not finite", who);
        for (int b = 0; b < n_amp_rows; b++) {
            const double amp = images[(IMAGE_ROWS + b) * n + i];
            if (!((zero_allowed ? amp >= 0.0 : amp > 0.0) && amp <= 1.0))
                return room_fail(-1, "%s: an image's amplitude is outside %s", who, zero_allowed ? "[0, 1]" : "(0, 1]");
        }
    }
    return 0;
}

inline int check_sources(const char *who, const double *sources, int n_sources)
{
    for (int r = 0; r < n_sources; r++) {
        const double *s = sources + (int64_t)SOURCE_COLS * r;
        if (!(fabs(s[0]) <= 1e9 && fabs(s[1]) <= 1e9 && fabs(s[2]) <= 1e9)) return room_fail(-1, "%s: a source position is not finite", who);
        if (!(s[3] >= 0.0 && s[3] <= 1e9 && s[3] == floor(s[3]))) return room_fail(-1, "%s: a time origin is not a whole number >= 0", who);
        if (!(s[4] > 0.0 && s[4] <= 1e9)) return room_fail(-1, "%s: a gain is not positive and finite", who);
    }
    return 0;
}

// what every gather takes: the counts, fs / c, the table, the sources, and last the n_points points (`what`: how a message calls one),
// copied into dst[n_dst][3] with zeros behind them
inline int check_common(const char *who, const double *images, int n_images, int n_amp_rows, bool zero_allowed, const double *sources,
                        int n_sources, double fs_over_c, const double *points, int n_points, const char *what, double *dst, int n_dst)
{
    if (n_images < 1 || n_images > MAX_IMAGES) return room_fail(-1, "%s: 1 .. %d images", who, MAX_IMAGES);
    if (n_sources < 1 || n_sources > MAX_SOURCES) return room_fail(-1, "%s: 1 .. %d sources", who, MAX_SOURCES);
    if (!(fs_over_c > 0.0 && fs_over_c <= 1e9)) return room_fail(-1, "%s: fs / c must be positive and finite", who);
    if (int rc = check_image_table(who, images, n_images, n_amp_rows, zero_allowed)) return rc;
    if (int rc = check_sources(who, sources, n_sources)) return rc;
    for (int e = 0; e < 3 * n_dst; e++) {
        dst[e] = e < 3 * n_points ? points[e] : 0.0;
        if (!(fabs(dst[e]) <= 1e9)) return room_fail(-1, "%s: %s is not finite", who, what);
    }
    return 0;
}

} // namespace room
