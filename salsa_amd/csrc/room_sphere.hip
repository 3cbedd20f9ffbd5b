// room_sphere.hip -- the MIC capsules of a shoebox room on a rigid sphere (include/salsa_hip.h: salsa_room_rirs_sphere; DESIGN.md
// section 9o).  The pressure of a plane wave from the unit direction u at a capsule at the unit direction m on a rigid sphere of radius
// R, relative to the free-field pressure at the centre, is H(f, Theta) = sum_n i^n (2 n + 1) b_n(k R) P_n(cos Theta), b_n(x) = j_n(x) -
// j_n'(x) / h_n^(2)'(x) h_n^(2)(x), cos Theta = u . m.  The host (salsa_amd/rooms.py: SphereTable) has turned it into a float32 table
// S[Q + 1][P + 1][LT], LT = lead + trail, of band-limited tap weights: uniform in Theta (row q is q pi / Q) and in the sub-sample phase
// (row p is p / P; row P is row 0 one tap on), j fastest.  An image adds
//     g (A / d) bilinear(S; Theta_m, frac tau)[k - floor(tau) + lead - 1]
// to tap k of capsule m, with d and tau measured to the array CENTRE: one distance and one delay for the four capsules, four angles.
//
//   sphere_kernel   room_kernel's gather (room_rir.hip), all four capsules in one workgroup: 256 consecutive taps of one source, one tap
//                   per thread, four accumulators.  The image table is walked in table order, 256 images at a time, one per thread:
//                   position, distance, delay, cos Theta and Theta of the four capsules in float64, once per image and not once per
//                   capsule.  An image whose taps floor(tau) - lead + 1 .. floor(tau) + trail meet the block is kept and compacted into
//                   LDS IN TABLE ORDER (ballot and popcount inside a wave, the waves' counts summed in wave order) as (floor tau, the
//                   phase weight, the float32 coefficient, per capsule the offset of the table row (q, p) and the angle weight): 44
//                   bytes.  Then every thread adds the kept images to its own tap, in that order, in float32: no atomics, nothing
//                   summed across threads, so two runs, and a source alone or in a batch, agree bit for bit.
//
// Table reads.  The 64 lanes of a wave are 64 consecutive taps, so for one entry they read 64 consecutive floats of each of the rows (q,
// p), (q, p + 1), (q + 1, p), (q + 1, p + 1): one coalesced request per row, four per capsule, sixteen per entry, in place of the open
// kernel's sinpif, cospif and division.  The table (1.9 MB at Q = 180, P = 32, LT = 79) stays in L2.  The entries are read by every lane
// at ONE address (an LDS broadcast).  All indices are clamped on the device as well: q to [0, Q - 1], p to [0, P - 1], j to [0, LT), so
// the largest offset read is (Q + 1)(P + 1) LT - 1 whatever the geometry gives (a NaN angle included).
//
// Precision split: p, d, tau, floor(tau), the fraction, cos Theta, Theta, both interpolation weights and the coefficient are float64,
// each rounded once; from the table lookup on everything is float32.  The launcher checks every argument and the host copy of the
// tables before the first device call; all output offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int SP_THREADS = 256, SP_WAVES = 4, SP_TAPS = 256;   // one tap per thread (salsa_room_tap_block())
constexpr int SP_CAPS = 4;
constexpr int SP_MAX_RIR = 16384, SP_MAX_IMAGES = 1 << 22, SP_MAX_SOURCES = 65535;
constexpr int SP_MAX_Q = 4096, SP_MAX_P = 1024, SP_MAX_SUPPORT = 512, SP_MAX_ENTRIES = 1 << 27;
constexpr int SP_SOURCE_COLS = 5;

struct sphere_args {
    double centre[3];
    double cap[SP_CAPS][3];
    double fs_over_c, q_per_rad;   // q_per_rad = Q / pi
    int n_images, rir_len, Q, P, lead, trail;
};

__global__ __launch_bounds__(SP_THREADS) void sphere_kernel(const double *__restrict__ images, const double *__restrict__ sources,
                                                            const float *__restrict__ table, const sphere_args a, float *__restrict__ out)
{
    __shared__ int s_k0[SP_THREADS], s_row[SP_THREADS][SP_CAPS];
    __shared__ float s_wp[SP_THREADS], s_c[SP_THREADS], s_wq[SP_THREADS][SP_CAPS];
    __shared__ int s_count[SP_WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = (int)blockIdx.z;
    const int lo = (int)blockIdx.x * SP_TAPS, hi = min(lo + SP_TAPS, a.rir_len);   // this block's taps [lo, hi)
    const int k = lo + tid;
    const int LT = a.lead + a.trail, pstride = LT, qstride = (a.P + 1) * LT;
    const double *src = sources + (int64_t)SP_SOURCE_COLS * r;
    const double sx = src[0], sy = src[1], sz = src[2], t0 = src[3], g = src[4];
    // floor(tau) of an image that reaches the block: its taps floor(tau) - lead + 1 .. floor(tau) + trail meet [lo, hi)
    const double f_lo = (double)(lo - a.trail), f_hi = (double)(hi + a.lead - 2);
    const int64_t n = a.n_images;
    float acc[SP_CAPS];
#pragma unroll
    for (int m = 0; m < SP_CAPS; m++) acc[m] = 0.f;

    for (int64_t base = 0; base < n; base += SP_THREADS) {
        const int64_t i = base + tid;
        bool hit = false;
        int k0 = 0, row[SP_CAPS];
        float wp = 0.f, co = 0.f, wq[SP_CAPS];
#pragma unroll
        for (int m = 0; m < SP_CAPS; m++) row[m] = 0, wq[m] = 0.f;
        if (i < n) {
            const double dx = images[i] * sx + images[3 * n + i] - a.centre[0];
            const double dy = images[n + i] * sy + images[4 * n + i] - a.centre[1];
            const double dz = images[2 * n + i] * sz + images[5 * n + i] - a.centre[2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            const double tau = d * a.fs_over_c - t0;
            const double tf = floor(tau);
            hit = tf >= f_lo && tf <= f_hi;               // (false for a NaN; bounds tf before it becomes an int)
            if (hit) {
                k0 = (int)tf;
                const double pf = (tau - tf) * (double)a.P;
                const int p = min(max((int)pf, 0), a.P - 1);
                wp = (float)(pf - (double)p);
                co = (float)(g * images[6 * n + i] / d);
#pragma unroll
                for (int m = 0; m < SP_CAPS; m++) {
                    const double c = fmin(fmax((dx * a.cap[m][0] + dy * a.cap[m][1] + dz * a.cap[m][2]) / d, -1.0), 1.0);
                    const double qf = acos(c) * a.q_per_rad;
                    const int q = min(max((int)qf, 0), a.Q - 1);
                    wq[m] = (float)(qf - (double)q);
                    row[m] = q * qstride + p * pstride;
                }
            }
        }
        // compaction in table order: the lanes before me in my wave, then the waves before mine
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s_count[w] = __popcll(mask);
        __syncthreads();
        int pos = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int v = 0; v < SP_WAVES; v++) {
            const int cv = s_count[v];
            pos += v < w ? cv : 0;
            total += cv;
        }
        if (hit) {
            s_k0[pos] = k0;
            s_wp[pos] = wp;
            s_c[pos] = co;
#pragma unroll
            for (int m = 0; m < SP_CAPS; m++) s_row[pos][m] = row[m], s_wq[pos][m] = wq[m];
        }
        __syncthreads();
        for (int e = 0; e < total; e++) {
            const int j = k - s_k0[e] + a.lead - 1;
            if (j < 0 || j >= LT) continue;
            const float fp = s_wp[e], cf = s_c[e];
#pragma unroll
            for (int m = 0; m < SP_CAPS; m++) {
                const float *t = table + s_row[e][m] + j;
                const float fq = s_wq[e][m];
                const float e0 = (1.f - fp) * t[0] + fp * t[pstride];
                const float e1 = (1.f - fp) * t[qstride] + fp * t[qstride + pstride];
                acc[m] += cf * ((1.f - fq) * e0 + fq * e1);
            }
        }
        __syncthreads();                                  // the entries and the counts are free for the next chunk
    }
    if (k >= hi) return;
#pragma unroll
    for (int m = 0; m < SP_CAPS; m++) out[((int64_t)r * SP_CAPS + m) * a.rir_len + k] = acc[m];
}

__attribute__((format(printf, 2, 3))) int sfail(int code, const char *fmt, ...)
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

extern "C" int salsa_room_sphere_limits(int *max_q, int *max_p, int *max_support)
{
    if (max_q) *max_q = SP_MAX_Q;
    if (max_p) *max_p = SP_MAX_P;
    if (max_support) *max_support = SP_MAX_SUPPORT;
    return SP_MAX_ENTRIES;
}

extern "C" int salsa_room_rirs_sphere(const double *images, const double *images_dev, int n_images, const double *sources,
                                      const double *sources_dev, int n_sources, const double *centre, const double *capsule_units,
                                      const float *table, const float *table_dev, int Q, int P, int lead, int trail, double fs_over_c,
                                      int rir_len, float *out, void *hip_stream)
{
    if (!images || !images_dev || !sources || !sources_dev || !centre || !capsule_units || !table || !table_dev || !out)
        return sfail(-1, "salsa_room_rirs_sphere: null pointer");
    if (Q < 1 || Q > SP_MAX_Q || P < 1 || P > SP_MAX_P) return sfail(-1, "salsa_room_rirs_sphere: 1 <= Q <= %d and 1 <= P <= %d", SP_MAX_Q, SP_MAX_P);
    if (lead < 1 || trail < 1 || lead > SP_MAX_SUPPORT || trail > SP_MAX_SUPPORT || lead + trail > SP_MAX_SUPPORT)
        return sfail(-1, "salsa_room_rirs_sphere: lead >= 1, trail >= 1 and lead + trail <= %d", SP_MAX_SUPPORT);
    const int64_t entries = (int64_t)(Q + 1) * (P + 1) * (lead + trail);
    if (entries > SP_MAX_ENTRIES) return sfail(-1, "salsa_room_rirs_sphere: the table has more than %d entries", SP_MAX_ENTRIES);
    if (n_images < 1 || n_images > SP_MAX_IMAGES) return sfail(-1, "salsa_room_rirs_sphere: 1 .. %d images", SP_MAX_IMAGES);
    if (n_sources < 1 || n_sources > SP_MAX_SOURCES) return sfail(-1, "salsa_room_rirs_sphere: 1 .. %d sources", SP_MAX_SOURCES);
    if (rir_len < 1 || rir_len > SP_MAX_RIR) return sfail(-1, "salsa_room_rirs_sphere: 1 <= rir length <= %d", SP_MAX_RIR);
    if (!(fs_over_c > 0.0 && fs_over_c <= 1e9)) return sfail(-1, "salsa_room_rirs_sphere: fs / c must be positive and finite");
    for (int64_t e = 0; e < entries; e++)
        if (!(fabsf(table[e]) <= 3e38f)) return sfail(-1, "salsa_room_rirs_sphere: a table entry is not finite");
    const int64_t n = n_images;
    for (int64_t i = 0; i < n; i++) {
        for (int ax = 0; ax < 3; ax++)
            if (fabs(images[ax * n + i]) != 1.0 || !(fabs(images[(3 + ax) * n + i]) <= 1e9))
                return sfail(-1, "salsa_room_rirs_sphere: an image's sign is not +-1 or its shift is not finite");
        if (!(images[6 * n + i] > 0.0 && images[6 * n + i] <= 1.0))
            return sfail(-1, "salsa_room_rirs_sphere: an image's amplitude is outside (0, 1]");
    }
    for (int r = 0; r < n_sources; r++) {
        const double *s = sources + (int64_t)SP_SOURCE_COLS * r;
        if (!(fabs(s[0]) <= 1e9 && fabs(s[1]) <= 1e9 && fabs(s[2]) <= 1e9)) return sfail(-1, "salsa_room_rirs_sphere: a source position is not finite");
        if (!(s[3] >= 0.0 && s[3] <= 1e9 && s[3] == floor(s[3]))) return sfail(-1, "salsa_room_rirs_sphere: a time origin is not a whole number >= 0");
        if (!(s[4] > 0.0 && s[4] <= 1e9)) return sfail(-1, "salsa_room_rirs_sphere: a gain is not positive and finite");
    }
    sphere_args a;
    for (int ax = 0; ax < 3; ax++) {
        a.centre[ax] = centre[ax];
        if (!(fabs(a.centre[ax]) <= 1e9)) return sfail(-1, "salsa_room_rirs_sphere: the centre is not finite");
    }
    for (int m = 0; m < SP_CAPS; m++) {
        double norm2 = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            a.cap[m][ax] = capsule_units[3 * m + ax];
            norm2 += a.cap[m][ax] * a.cap[m][ax];
        }
        if (!(fabs(norm2 - 1.0) <= 2e-6)) return sfail(-1, "salsa_room_rirs_sphere: a capsule direction is not a unit vector");
    }
    a.fs_over_c = fs_over_c;
    a.q_per_rad = (double)Q / 3.14159265358979323846;
    a.n_images = n_images;
    a.rir_len = rir_len;
    a.Q = Q;
    a.P = P;
    a.lead = lead;
    a.trail = trail;
    const dim3 grid((unsigned)((rir_len + SP_TAPS - 1) / SP_TAPS), 1u, (unsigned)n_sources);
    hipLaunchKernelGGL(sphere_kernel, grid, dim3(SP_THREADS), 0, (hipStream_t)hip_stream, images_dev, sources_dev, table_dev, a, out);
    return hipGetLastError() == hipSuccess ? 0 : sfail(-6, "salsa_room_rirs_sphere: launch failed");
}
