// nn_pool.hip -- gfx950 kernels for the pooling layers of the SELD CRNN (C ABI: include/salsa_nn.h): the 2x2 average pool and
// the decoder's mean / max / mean + max over the frequency axis.  Streaming passes: 16-byte accesses, channels-last so that a
// thread's vector is contiguous.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>

#include "../../include/salsa_nn.h"
#include "nn_vec.h"

namespace {

// one thread = one output pixel x L channels (16 bytes); x, y channels-last
template <typename V, int L>
__global__ __launch_bounds__(256) void avgpool2x2_fwd_kernel(const char *__restrict__ x, char *__restrict__ y, long n_vec,
                                                             int H, int W, int C)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const int cv = C / L, Ho = H / 2, Wo = W / 2;
    const int c = (int)(i % cv);
    long r = i / cv;
    const int wo = (int)(r % Wo);
    r /= Wo;
    const int ho = (int)(r % Ho);
    const long n = r / Ho;
    const long esz = 16 / L; // bytes per element
    const char *p = x + (((n * H + 2 * ho) * W + 2 * wo) * C + (long)c * L) * esz;
    float a[L], b[L], cc[L], d[L], o[L];
    vec_io<V, L>::load(p, a);
    vec_io<V, L>::load(p + (long)C * esz, b);
    vec_io<V, L>::load(p + (long)W * C * esz, cc);
    vec_io<V, L>::load(p + ((long)W * C + C) * esz, d);
#pragma unroll
    for (int k = 0; k < L; k++) o[k] = (((a[k] + b[k]) + cc[k]) + d[k]) / 4.0f; // the reference implementation's order
    vec_io<V, L>::store(y + i * 16, o);
}

// one thread = one INPUT pixel x L channels: grad_x = grad_y[h/2][w/2] / 4, zero in a dropped odd row / column
template <typename V, int L>
__global__ __launch_bounds__(256) void avgpool2x2_bwd_kernel(const char *__restrict__ gy, char *__restrict__ gx, long n_vec,
                                                             int H, int W, int C)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_vec) return;
    const int cv = C / L, Ho = H / 2, Wo = W / 2;
    const int c = (int)(i % cv);
    long r = i / cv;
    const int w = (int)(r % W);
    r /= W;
    const int h = (int)(r % H);
    const long n = r / H;
    float g[L];
    if (h < 2 * Ho && w < 2 * Wo) {
        vec_io<V, L>::load(gy + ((((n * Ho + h / 2) * Wo + w / 2) * cv + c) * 16), g);
#pragma unroll
        for (int k = 0; k < L; k++) g[k] = g[k] / 4.0f;
    } else {
#pragma unroll
        for (int k = 0; k < L; k++) g[k] = 0.f;
    }
    vec_io<V, L>::store(gx + i * 16, g);
}

// ------------------------------------------------------------------------------------------------------------ frequency mean
// The decoder's first step (models/decoders.py: x.mean(dim=3), then (B, C, T) -> (B, T, C)): x bf16 channels-last [N][H][W][C]
// -> float32 [H][N][C] (time-major, the GRU's order) or [N][H][C]; torch's reduction over the strided axis ran at 0.4 TB/s.
__global__ __launch_bounds__(256) void freq_mean_fwd_kernel(const unsigned short *__restrict__ x, float *__restrict__ y, long rows,
                                                            int N, int H, int W, int C, int time_major)
{
    const int cv = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cv) return;
    const long r = i / cv;
    const int c8 = (int)(i - r * cv);
    const uint4 *p = (const uint4 *)(x + (r * W) * C + c8 * 8);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < W; w++) {
        const uint4 v = p[(long)w * cv];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            acc[2 * k] += __uint_as_float(u[k] << 16);
            acc[2 * k + 1] += __uint_as_float(u[k] & 0xFFFF0000u);
        }
    }
    const float inv = 1.f / (float)W;
    const long n = r / H, h = r - n * H;
    float *o = y + ((time_major ? h * N + n : r) * C + c8 * 8);
    *(float4 *)o = make_float4(acc[0] * inv, acc[1] * inv, acc[2] * inv, acc[3] * inv);
    *(float4 *)(o + 4) = make_float4(acc[4] * inv, acc[5] * inv, acc[6] * inv, acc[7] * inv);
}

// dx[n][h][w][c] = g[row(n, h)][c] / W, bf16 channels-last
__global__ __launch_bounds__(256) void freq_mean_bwd_kernel(const float *__restrict__ g, unsigned short *__restrict__ dx, long rows,
                                                            int N, int H, int W, int C, int time_major)
{
    const int cv = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * W * cv) return;
    const long rw = i / cv;
    const int c8 = (int)(i - rw * cv);
    const long r = rw / W;
    const long n = r / H, h = r - n * H;
    const float *src = g + ((time_major ? h * N + n : r) * C + c8 * 8);
    const float4 a = *(const float4 *)src, b = *(const float4 *)(src + 4);
    const float inv = 1.f / (float)W;
    uint4 o;
    o.x = pack_bf16(a.x * inv, a.y * inv);
    o.y = pack_bf16(a.z * inv, a.w * inv);
    o.z = pack_bf16(b.x * inv, b.y * inv);
    o.w = pack_bf16(b.z * inv, b.w * inv);
    *(uint4 *)(dx + rw * C + c8 * 8) = o;
}

// ------------------------------------------------------------------------------------------- frequency max / avg + max pool
// The decoder's freq_pool 'max' and 'avg_max' (models/decoders.py: torch.max(x, dim=3), mean + max) in one pass, laid out like
// freq_mean_fwd_kernel (8 channels per thread).  mode 1: y = max; mode 2: y = mean + max, the mean accumulated in w order as
// freq_mean does.  argmax (uint8, W <= 255) is the LOWEST w holding the maximum; a NaN wins over every number and the first NaN
// is kept, so NaN propagates with its own index.
__global__ __launch_bounds__(256) void freq_pool_fwd_kernel(const unsigned short *__restrict__ x, float *__restrict__ y,
                                                            uint8_t *__restrict__ argmax, long rows, int N, int H, int W, int C,
                                                            int mode, int time_major)
{
    const int cv = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cv) return;
    const long r = i / cv;
    const int c8 = (int)(i - r * cv);
    const uint4 *p = (const uint4 *)(x + (r * W) * C + c8 * 8);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, mx[8];
    int am[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < W; w++) {
        const uint4 v = p[(long)w * cv];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
        float e[8];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            e[2 * k] = __uint_as_float(u[k] << 16);
            e[2 * k + 1] = __uint_as_float(u[k] & 0xFFFF0000u);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc[k] += e[k];
            const bool take = w == 0 || e[k] > mx[k] || (e[k] != e[k] && mx[k] == mx[k]); // strictly greater, or the first NaN
            mx[k] = take ? e[k] : mx[k];
            am[k] = take ? w : am[k];
        }
    }
    const float inv = 1.f / (float)W;
    float out[8];
#pragma unroll
    for (int k = 0; k < 8; k++) out[k] = mode == 2 ? __fadd_rn(__fmul_rn(acc[k], inv), mx[k]) : mx[k]; // (mean rounded, then added: no fma)
    const long n = r / H, h = r - n * H;
    const long row = time_major ? h * N + n : r;
    float *o = y + (row * C + c8 * 8);
    *(float4 *)o = make_float4(out[0], out[1], out[2], out[3]);
    *(float4 *)(o + 4) = make_float4(out[4], out[5], out[6], out[7]);
    uint2 a;
    a.x = (unsigned)am[0] | ((unsigned)am[1] << 8) | ((unsigned)am[2] << 16) | ((unsigned)am[3] << 24);
    a.y = (unsigned)am[4] | ((unsigned)am[5] << 8) | ((unsigned)am[6] << 16) | ((unsigned)am[7] << 24);
    *(uint2 *)(argmax + row * C + c8 * 8) = a;
}

// dx[n][h][w][c] = g[row][c] / W (mode 2 only) + g[row][c] * (w == argmax[row][c]), bf16 channels-last
__global__ __launch_bounds__(256) void freq_pool_bwd_kernel(const float *__restrict__ g, const uint8_t *__restrict__ argmax,
                                                            unsigned short *__restrict__ dx, long rows, int N, int H, int W, int C,
                                                            int mode, int time_major)
{
    const int cv = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * W * cv) return;
    const long rw = i / cv;
    const int c8 = (int)(i - rw * cv);
    const long r = rw / W;
    const int w = (int)(rw - r * W);
    const long n = r / H, h = r - n * H;
    const long row = time_major ? h * N + n : r;
    const float *src = g + (row * C + c8 * 8);
    const float4 a = *(const float4 *)src, b = *(const float4 *)(src + 4);
    const uint2 am = *(const uint2 *)(argmax + row * C + c8 * 8);
    const float gv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const float inv = mode == 2 ? 1.f / (float)W : 0.f;
    float d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int idx = (int)(((k < 4 ? am.x : am.y) >> (8 * (k & 3))) & 0xFFu);
        d[k] = __fadd_rn(__fmul_rn(gv[k], inv), idx == w ? gv[k] : 0.f);
    }
    uint4 o;
    o.x = pack_bf16(d[0], d[1]);
    o.y = pack_bf16(d[2], d[3]);
    o.z = pack_bf16(d[4], d[5]);
    o.w = pack_bf16(d[6], d[7]);
    *(uint4 *)(dx + rw * C + c8 * 8) = o;
}

} // namespace

extern "C" {

int salsa_nn_avgpool2x2_fwd(const void *x, void *y, int dtype, int64_t N, int H, int W, int C, void *hip_stream)
{
    const int L = dtype == 1 ? 8 : 4;
    if (!x || !y || N <= 0 || H < 2 || W < 2 || C <= 0 || C % L || (dtype != 0 && dtype != 1)) return -1;
    const long n_vec = (long)N * (H / 2) * (W / 2) * (C / L);
    const dim3 grid((unsigned)((n_vec + 255) / 256));
    if (dtype == 1)
        hipLaunchKernelGGL((avgpool2x2_fwd_kernel<bf16x8, 8>), grid, dim3(256), 0, (hipStream_t)hip_stream, (const char *)x, (char *)y, n_vec, H, W, C);
    else
        hipLaunchKernelGGL((avgpool2x2_fwd_kernel<f32x4, 4>), grid, dim3(256), 0, (hipStream_t)hip_stream, (const char *)x, (char *)y, n_vec, H, W, C);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

int salsa_nn_avgpool2x2_bwd(const void *grad_y, void *grad_x, int dtype, int64_t N, int H, int W, int C, void *hip_stream)
{
    const int L = dtype == 1 ? 8 : 4;
    if (!grad_y || !grad_x || N <= 0 || H < 2 || W < 2 || C <= 0 || C % L || (dtype != 0 && dtype != 1)) return -1;
    const long n_vec = (long)N * H * W * (C / L);
    const dim3 grid((unsigned)((n_vec + 255) / 256));
    if (dtype == 1)
        hipLaunchKernelGGL((avgpool2x2_bwd_kernel<bf16x8, 8>), grid, dim3(256), 0, (hipStream_t)hip_stream, (const char *)grad_y, (char *)grad_x, n_vec, H, W, C);
    else
        hipLaunchKernelGGL((avgpool2x2_bwd_kernel<f32x4, 4>), grid, dim3(256), 0, (hipStream_t)hip_stream, (const char *)grad_y, (char *)grad_x, n_vec, H, W, C);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* mean over the frequency axis of a bf16 channels-last map x [N][H][W][C] -> float32 y, [H][N][C] when time_major else [N][H][C];
 * C % 8 == 0.  _bwd: dx = g / W broadcast over W, bf16 channels-last. */
int salsa_nn_freq_mean_fwd(const void *x, float *y, int64_t N, int H, int W, int C, int time_major, void *hip_stream)
{
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return -1;
    const long rows = (long)N * H, n = rows * (C / 8);
    hipLaunchKernelGGL(freq_mean_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const unsigned short *)x, y, rows, (int)N, H, W, C, time_major);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

int salsa_nn_freq_mean_bwd(const float *g, void *dx, int64_t N, int H, int W, int C, int time_major, void *hip_stream)
{
    if (!g || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return -1;
    const long rows = (long)N * H, n = rows * W * (C / 8);
    hipLaunchKernelGGL(freq_mean_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, g,
                       (unsigned short *)dx, rows, (int)N, H, W, C, time_major);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* frequency max (mode 1) / mean + max (mode 2) of a bf16 channels-last map x [N][H][W][C] -> float32 y and uint8 argmax, both
 * [H][N][C] when time_major else [N][H][C]; C % 8 == 0, W <= 255.  _bwd: dx = g / W (mode 2) + g at w == argmax, bf16 channels-last. */
int salsa_nn_freq_pool_fwd(const void *x, float *y, uint8_t *argmax, int64_t N, int H, int W, int C, int mode, int time_major,
                           void *hip_stream)
{
    if (!x || !y || !argmax || N <= 0 || H <= 0 || W <= 0 || W > 255 || C <= 0 || C % 8 || (mode != 1 && mode != 2)) return -1;
    const long rows = (long)N * H, n = rows * (C / 8);
    hipLaunchKernelGGL(freq_pool_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream,
                       (const unsigned short *)x, y, argmax, rows, (int)N, H, W, C, mode, time_major);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

int salsa_nn_freq_pool_bwd(const float *g, const uint8_t *argmax, void *dx, int64_t N, int H, int W, int C, int mode, int time_major,
                           void *hip_stream)
{
    if (!g || !argmax || !dx || N <= 0 || H <= 0 || W <= 0 || W > 255 || C <= 0 || C % 8 || (mode != 1 && mode != 2)) return -1;
    const long rows = (long)N * H, n = rows * W * (C / 8);
    hipLaunchKernelGGL(freq_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, g, argmax,
                       (unsigned short *)dx, rows, (int)N, H, W, C, mode, time_major);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

} // extern "C"
