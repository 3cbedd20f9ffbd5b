// room_sphere.hip -- the MIC capsules of a shoebox room on a rigid sphere (include/salsa_hip.h: salsa_room_rirs_sphere; DESIGN.md
// section 9o).  The pressure of a plane wave from the unit direction u at a capsule at the unit direction m on a rigid sphere of radius
// R, relative to the free-field pressure at the centre, is H(f, Theta) = sum_n i^n (2 n + 1) b_n(k R) P_n(cos Theta), b_n(x) = j_n(x) -
// j_n'(x) / h_n^(2)'(x) h_n^(2)(x), cos Theta = u . m.  The host (salsa_amd/rooms.py: SphereTable) has turned it into a float32 table
// S[Q + 1][P + 1][LT], LT = lead + trail, of band-limited tap weights: uniform in Theta (row q is q pi / Q) and in the sub-sample phase
// (row p is p / P; row P is row 0 one tap on), j fastest.  An image adds
//     g (A / d) bilinear(S; Theta_m, frac tau)[k - floor(tau) + lead - 1]
// to tap k of capsule m, with d and tau measured to the array CENTRE: one distance and one delay for the four capsules, four angles.
//
//   sphere_kernel   room_gather.h's skeleton, all four capsules in one workgroup: 256 consecutive taps of one source, one tap per thread,
//                   four accumulators.  Position, distance and delay are the shared geometry, measured to the centre; cos Theta and Theta
//                   of the four capsules follow in float64, once per image and not once per capsule.  An image whose taps floor(tau) -
//                   lead + 1 .. floor(tau) + trail meet the block is kept and compacted as (floor tau, the phase weight, the float32
//                   coefficient, per capsule the offset of the table row (q, p) and the angle weight): 44 bytes.
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
#include <stdint.h>
#include "../../include/salsa_hip.h"
#include "room_gather.h"

namespace {

using namespace room;

constexpr int SP_CAPS = 4;
constexpr int SP_MAX_Q = 4096, SP_MAX_P = 1024, SP_MAX_SUPPORT = 512, SP_MAX_ENTRIES = 1 << 27;

struct sphere_args {
    double centre[3];
    double cap[SP_CAPS][3];
    double fs_over_c, q_per_rad;   // q_per_rad = Q / pi
    int n_images, rir_len, Q, P, lead, trail;
};

__global__ __launch_bounds__(THREADS) void sphere_kernel(const double *__restrict__ images, const double *__restrict__ sources,
                                                         const float *__restrict__ table, const sphere_args a, float *__restrict__ out)
{
    __shared__ int s_k0[THREADS], s_row[THREADS][SP_CAPS];
    __shared__ float s_wp[THREADS], s_c[THREADS], s_wq[THREADS][SP_CAPS];
    __shared__ int s_count[WAVES];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = (int)blockIdx.z;
    const int lo = (int)blockIdx.x * TAPS, hi = min(lo + TAPS, a.rir_len);   // this block's taps [lo, hi)
    const int k = lo + tid;
    const int LT = a.lead + a.trail, pstride = LT, qstride = (a.P + 1) * LT;
    const source_row s = load_source(sources, r);
    // floor(tau) of an image that reaches the block: its taps floor(tau) - lead + 1 .. floor(tau) + trail meet [lo, hi)
    const double f_lo = (double)(lo - a.trail), f_hi = (double)(hi + a.lead - 2);
    const int64_t n = a.n_images;
    float acc[SP_CAPS];
#pragma unroll
    for (int m = 0; m < SP_CAPS; m++) acc[m] = 0.f;

    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + tid;
        bool hit = false;
        int k0 = 0, row[SP_CAPS];
        float wp = 0.f, co = 0.f, wq[SP_CAPS];
#pragma unroll
        for (int m = 0; m < SP_CAPS; m++) row[m] = 0, wq[m] = 0.f;
        if (i < n) {
            const image_path ip = image_geometry(images, n, i, s, a.centre[0], a.centre[1], a.centre[2], a.fs_over_c);
            hit = image_reaches(ip.tf, f_lo, f_hi);
            if (hit) {
                k0 = (int)ip.tf;
                const double pf = (ip.tau - ip.tf) * (double)a.P;
                const int p = min(max((int)pf, 0), a.P - 1);
                wp = (float)(pf - (double)p);
                co = (float)image_gain(images, n, i, 0, s.g, ip.d);
#pragma unroll
                for (int m = 0; m < SP_CAPS; m++) {
                    const double c = fmin(fmax((ip.dx * a.cap[m][0] + ip.dy * a.cap[m][1] + ip.dz * a.cap[m][2]) / ip.d, -1.0), 1.0);
                    const double qf = acos(c) * a.q_per_rad;
                    const int q = min(max((int)qf, 0), a.Q - 1);
                    wq[m] = (float)(qf - (double)q);
                    row[m] = q * qstride + p * pstride;
                }
            }
        }
        int pos, total;
        compact(hit, s_count, lane, w, pos, total);
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
    const char *who = "salsa_room_rirs_sphere";
    if (!images || !images_dev || !sources || !sources_dev || !centre || !capsule_units || !table || !table_dev || !out)
        return room_fail(-1, "%s: null pointer", who);
    if (Q < 1 || Q > SP_MAX_Q || P < 1 || P > SP_MAX_P) return room_fail(-1, "%s: 1 <= Q <= %d and 1 <= P <= %d", who, SP_MAX_Q, SP_MAX_P);
    if (lead < 1 || trail < 1 || lead > SP_MAX_SUPPORT || trail > SP_MAX_SUPPORT || lead + trail > SP_MAX_SUPPORT)
        return room_fail(-1, "%s: lead >= 1, trail >= 1 and lead + trail <= %d", who, SP_MAX_SUPPORT);
    const int64_t entries = (int64_t)(Q + 1) * (P + 1) * (lead + trail);
    if (entries > SP_MAX_ENTRIES) return room_fail(-1, "%s: the table has more than %d entries", who, SP_MAX_ENTRIES);
    if (rir_len < 1 || rir_len > MAX_RIR) return room_fail(-1, "%s: 1 <= rir length <= %d", who, MAX_RIR);
    for (int64_t e = 0; e < entries; e++)
        if (!(fabsf(table[e]) <= 3e38f)) return room_fail(-1, "%s: a table entry is not finite", who);
    sphere_args a;
    if (int rc = check_common(who, images, n_images, 1, false, sources, n_sources, fs_over_c, centre, 1, "the centre", a.centre, 1)) return rc;
    for (int m = 0; m < SP_CAPS; m++) {
        double norm2 = 0.0;
        for (int ax = 0; ax < 3; ax++) {
            a.cap[m][ax] = capsule_units[3 * m + ax];
            norm2 += a.cap[m][ax] * a.cap[m][ax];
        }
        if (!(fabs(norm2 - 1.0) <= 2e-6)) return room_fail(-1, "%s: a capsule direction is not a unit vector", who);
    }
    a.fs_over_c = fs_over_c;
    a.q_per_rad = (double)Q / 3.14159265358979323846;
    a.n_images = n_images;
    a.rir_len = rir_len;
    a.Q = Q;
    a.P = P;
    a.lead = lead;
    a.trail = trail;
    const dim3 grid((unsigned)((rir_len + TAPS - 1) / TAPS), 1u, (unsigned)n_sources);
    hipLaunchKernelGGL(sphere_kernel, grid, dim3(THREADS), 0, (hipStream_t)hip_stream, images_dev, sources_dev, table_dev, a, out);
    return hipGetLastError() == hipSuccess ? 0 : room_fail(-6, "%s: launch failed", who);
}
