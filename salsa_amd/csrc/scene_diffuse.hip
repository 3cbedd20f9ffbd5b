// scene_diffuse.hip -- spatially diffuse ambient noise for the rendered scenes (include/salsa_hip.h: salsa_scene_diffuse,
// salsa_scene_diffuse_supported, salsa_scene_diffuse_block; salsa_amd/ambient.py).
// D uncorrelated plane-wave noises reach the four channels through the array's direct-path response `mix`, one colouring filter follows:
//     m[c][t] = sum_{d < D} sum_{k < La} mix[d][c][k] white(seed_b, d, t - k)        fmaf chain from +0, d outer, k inner, ascending
//     y[c][n] = sum_{j < Lg} colour[j] m[c][n - j]                                    fmaf chain from +0, j ascending
//     out[b][c][n] = fmaf(scale_b, y[c][n], in[b][c][n])     (without in: scale_b * y[c][n])
//
// white(seed, d, n), n >= -1024, is a pure function of its three integers, the splitmix64 sequence read at a counter (drop_hash's idea --
// a multiply-xorshift finaliser over a Weyl counter -- in 64 bits):
//     mix64(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31        (mod 2^64)
//     key = mix64(seed + 0x9E3779B97F4A7C15)
//     h   = mix64(key + ((d << 48) | (n + 1024)) * 0x9E3779B97F4A7C15)
//     white = (float)(u_0 + u_1 + u_2 + u_3 - 131070) * 0x1.bb67aep-16f,   u_i = (h >> 16 i) & 0xFFFF
// d < 2^8 and n + 1024 < 2^48 give every (d, n) a counter of its own, the multiplier is odd and mix64 is a bijection, so under one seed no two
// (d, n) share an h.  The sum of four 16-bit fields is Irwin-Hall of four: mean 0, variance 1 after the scale float32(sqrt(3 / (2^32 - 1)));
// the integer is below 2^24, so its conversion is exact and the product rounds once.  No transcendental: numpy restates it bit for bit
// (tests/diffuse_reference.py).
//
//   diffuse_kernel   one workgroup of 256 threads = BLOCK = 2048 output samples of one clip, all four channels.  It needs m on the BLOCK +
//                    Lg - 1 samples from n0 - (Lg - 1) on, and white on La - 1 more before them.  For each direction the stretch of white
//                    goes into LDS (two buffers: direction d + 1 is hashed while d is consumed, ONE barrier per direction); thread t
//                    owns the m samples t, t + 256, ... (at most 10) of all four channels in registers -- consecutive lanes read
//                    consecutive LDS words, the four mix taps are uniform and come through the scalar cache.  After the last direction m
//                    replaces white in the same LDS, and thread t runs the colour chain of the samples 4 t .. 4 t + 3 (then + 1024) from
//                    16-byte LDS reads: a group of four taps of four neighbouring samples touches seven consecutive m values, the upper
//                    four of which the previous group already holds, so 64 fmaf follow four ds_read_b128.
// Every m and y is a function of (seed_b, absolute sample) alone: the bits do not depend on the batch, the clip's place in it, the block
// or n_samples; no atomics, no global scratch, nothing stored between calls.  A clip of scale 0 copies `in` (or writes +0.0).
// LDS: 41 KiB, three workgroups per CU; about 80 VGPRs.  All output offsets are 64-bit.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/salsa_hip.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

namespace {

constexpr int THREADS = 256, BLOCK = 2048, NC = 4;
constexpr int MAX_DIRS = 256, MAX_MIX = 128, MAX_COLOUR = 513;
constexpr int64_t MAX_SAMPLES = (int64_t)1 << 32;               // exclusive: 2^40 / 256
constexpr int M_MAX = BLOCK + MAX_COLOUR - 1;                   // m samples of a block
constexpr int MI = (M_MAX + THREADS - 1) / THREADS;             // ... per thread
constexpr int W_STRIDE = (M_MAX + MAX_MIX - 1 + 3) / 4 * 4;     // white samples of a block and direction, one of two buffers
constexpr int M_STRIDE = M_MAX + 8;                             // one channel of m: up to 6 words of front padding, a multiple of 4
constexpr int SMEM = NC * M_STRIDE > 2 * W_STRIDE ? NC * M_STRIDE : 2 * W_STRIDE;
constexpr int WHITE_LEAD = 1024;                                // white is defined from -WHITE_LEAD on (>= MAX_MIX + MAX_COLOUR)
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ float white(uint64_t key, int d, int64_t n)
{
    const uint64_t h = mix64(key + (((uint64_t)d << 48) | (uint64_t)(n + WHITE_LEAD)) * GOLDEN);
    const unsigned lo = (unsigned)h, hi = (unsigned)(h >> 32);
    const int sum = (int)((lo & 0xFFFFu) + (lo >> 16) + (hi & 0xFFFFu) + (hi >> 16)) - 131070;
    return (float)sum * 0x1.bb67aep-16f;
}

typedef float f4 __attribute__((ext_vector_type(4)));

// four consecutive LDS words from a 16-byte boundary: one ds_read_b128
__device__ __forceinline__ f4 lds_quad(const float *p) { return *reinterpret_cast<const f4 *>(__builtin_assume_aligned(p, 16)); }

// NT taps j0 .. j0 + NT - 1 on four neighbouring samples of one channel: sample s, tap j0 + e reads w[4 + s - e], w = (lo, hi)
template <int NT>
__device__ __forceinline__ void colour_taps(float (&y)[4], const f4 lo, const f4 hi, const float *__restrict__ colour, int j0)
{
    const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int e = 0; e < NT; e++) {
        const float g = colour[j0 + e];
#pragma unroll
        for (int s = 0; s < 4; s++) y[s] = fmaf(g, w[4 + s - e], y[s]);
    }
}

__global__ __launch_bounds__(THREADS) void diffuse_kernel(const float *__restrict__ mix, int D, int La, const float *__restrict__ colour, int Lg,
                                                          const uint64_t *__restrict__ seeds, const float *__restrict__ scales,
                                                          const float *in, float *out, int64_t N, unsigned blocks_per_clip)
{
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    const int tid = (int)threadIdx.x;
    const unsigned b = blockIdx.x / blocks_per_clip;
    const int64_t n0 = (int64_t)(blockIdx.x - b * blocks_per_clip) * BLOCK;
    const int64_t base = (int64_t)b * NC * N;
    const float scale = scales[b];
    if (scale == 0.f) {                                          // the clip gets no noise: its input, or +0.0
        if (in == out) return;
        for (int c = 0; c < NC; c++)
            for (int o = tid; o < BLOCK && n0 + o < N; o += THREADS) {
                const int64_t at = base + c * N + n0 + o;
                out[at] = in ? in[at] : 0.f;
            }
        return;
    }
    const int mtot = BLOCK + Lg - 1, wtot = mtot + La - 1;
    const uint64_t key = mix64(seeds[b] + GOLDEN);
    const int64_t w0 = n0 - (Lg - 1) - (La - 1);                 // the sample of white's LDS word 0; m's word 0 is sample n0 - (Lg - 1)
    float acc[MI][NC];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int c = 0; c < NC; c++) acc[i][c] = 0.f;

    for (int l = tid; l < wtot; l += THREADS) smem[l] = white(key, 0, w0 + l);
    __syncthreads();
    for (int d = 0; d < D; d++) {
        const float *cur = smem + (d & 1) * W_STRIDE;
        if (d + 1 < D) {                                         // the other buffer was last read before the previous barrier
            float *nxt = smem + ((d + 1) & 1) * W_STRIDE;
            for (int l = tid; l < wtot; l += THREADS) nxt[l] = white(key, d + 1, w0 + l);
        }
        const float *mx = mix + (int64_t)d * NC * La;
        for (int k = 0; k < La; k++) {
            const float g0 = mx[k], g1 = mx[La + k], g2 = mx[2 * La + k], g3 = mx[3 * La + k];
            const float *wp = cur + (La - 1 - k) + tid;         // m sample p reads white word p + La - 1 - k
#pragma unroll
            for (int i = 0; i < MI; i++) {
                if (i < BLOCK / THREADS || tid + i * THREADS < mtot) {
                    const float w = wp[i * THREADS];
                    acc[i][0] = fmaf(g0, w, acc[i][0]);
                    acc[i][1] = fmaf(g1, w, acc[i][1]);
                    acc[i][2] = fmaf(g2, w, acc[i][2]);
                    acc[i][3] = fmaf(g3, w, acc[i][3]);
                }
            }
        }
        __syncthreads();
    }
    // m into LDS over white (the last barrier freed it).  The front padding puts output sample 4 t's newest tap on a 16-byte boundary
    // and leaves one whole quad below the oldest tap of the block's first sample.
    const int front = 4 + ((4 - ((Lg - 1) & 3)) & 3);
#pragma unroll
    for (int i = 0; i < MI; i++) {
        const int p = tid + i * THREADS;
        if (p < mtot) {
#pragma unroll
            for (int c = 0; c < NC; c++) smem[c * M_STRIDE + front + p] = acc[i][c];
        }
    }
    __syncthreads();
    for (int g = 0; g < BLOCK / (4 * THREADS); g++) {
        const int o = (g * THREADS + tid) * 4;
        if (n0 + o >= N) continue;
        const int a = o + (Lg - 1) + front;                      // a multiple of 4: the word of sample o's tap 0
        float y[NC][4];
        f4 hi[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            hi[c] = lds_quad(&smem[c * M_STRIDE + a]);
#pragma unroll
            for (int s = 0; s < 4; s++) y[c][s] = 0.f;
        }
        int j0 = 0;
        for (; j0 + 4 <= Lg; j0 += 4) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const f4 lo = lds_quad(&smem[c * M_STRIDE + a - j0 - 4]);
                colour_taps<4>(y[c], lo, hi[c], colour, j0);
                hi[c] = lo;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {                           // Lg is odd: one or three taps are left
            const f4 lo = lds_quad(&smem[c * M_STRIDE + a - j0 - 4]);
            if (Lg - j0 == 3)
                colour_taps<3>(y[c], lo, hi[c], colour, j0);
            else
                colour_taps<1>(y[c], lo, hi[c], colour, j0);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                if (n0 + o + s < N) {
                    const int64_t at = base + c * N + n0 + o + s;
                    out[at] = in ? fmaf(scale, y[c][s], in[at]) : scale * y[c][s];
                }
            }
        }
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

extern "C" int salsa_scene_diffuse_block(void) { return BLOCK; }

extern "C" int salsa_scene_diffuse_supported(int n_channels, int n_dirs, int mix_taps, int colour_taps)
{
    return n_channels == NC && n_dirs >= 1 && n_dirs <= MAX_DIRS && mix_taps >= 1 && mix_taps <= MAX_MIX && colour_taps >= 1
                   && colour_taps <= MAX_COLOUR && (colour_taps & 1)
               ? 1
               : 0;
}

extern "C" int salsa_scene_diffuse(const float *d_mix, int n_dirs, int n_channels, int mix_taps, const float *d_colour, int colour_taps,
                                   const uint64_t *d_seeds, const float *d_scales, const float *d_in, float *d_out, int n_clips,
                                   int64_t n_samples, void *hip_stream)
{
    const char *who = "salsa_scene_diffuse";
    if (!d_mix || !d_colour || !d_seeds || !d_scales || !d_out) return dfail(-1, "%s: null pointer", who);
    if (!salsa_scene_diffuse_supported(n_channels, n_dirs, mix_taps, colour_taps))
        return dfail(-1, "%s: %d channels, 1 .. %d directions, 1 .. %d mix taps, an odd number of 1 .. %d colour taps", who, NC, MAX_DIRS, MAX_MIX,
                     MAX_COLOUR);
    if (n_clips < 1 || n_samples < 1 || n_samples >= MAX_SAMPLES) return dfail(-1, "%s: n_clips >= 1 and 1 <= n_samples < 2^32", who);
    const int64_t per_clip = (n_samples + BLOCK - 1) / BLOCK;
    if (per_clip * n_clips > 0x7fffffffll) return dfail(-1, "%s: more than 2^31 - 1 blocks of %d samples", who, BLOCK);
    hipLaunchKernelGGL(diffuse_kernel, dim3((unsigned)(per_clip * n_clips)), dim3(THREADS), 0, (hipStream_t)hip_stream, d_mix, n_dirs, mix_taps,
                       d_colour, colour_taps, d_seeds, d_scales, d_in, d_out, n_samples, (unsigned)per_clip);
    return hipGetLastError() == hipSuccess ? 0 : dfail(-6, "%s: launch failed", who);
}
