// conformer.hip -- what a Conformer block after the recurrent decoder needs beside its GEMMs and the attention core (include/salsa_nn.h;
// DESIGN.md section 9r): the pre-norm residual step, the feed-forward epilogue and the convolution module, each with its backward.
// All float32, no atomics, every sum in a fixed order: bit-reproducible for a given shape, and a sample's result does not depend on the
// rest of the batch (but for the dropout masks, which depend on the element's flat index).
//
// Dropout.  DropArgs / drop_hash / drop_args of nn_common.h as the element-wise BatchNorm dropout uses them: p quantised to 1 / 65536,
// one 32-bit hash of (flat index >> 1, seed) serves two neighbouring elements (low 16 bits the even one), dropped when its 16 bits are
// below the threshold.  No mask is stored: the backward regenerates it from (p, seed).
//
// res_layernorm.  One wave per row (C = 256 or 512: one or two float4 per lane): z = x + scale * (branch * dropscale) where kept, x
// where dropped; the statistics are add_layernorm_fwd_kernel's (attention.hip) operation for operation, so scale 1, p 0 gives its
// bits.  Backward: the row-per-wave walk over a fixed grid, z recomputed from x, branch and the mask, per-lane dgamma / dbeta partial
// sums added in wave order into the workgroup's slab, the slabs added in slab order by a second launch.
//
// bias_swish_dropout.  Element-wise forward, one float4 per thread.  Backward: a wave owns 64 float4 columns and walks rows; the
// four waves of a workgroup are added in wave order into the workgroup's slab of the bias gradient, slabs added in slab order.
//
// conv_module.  u = swish(LN(DW(glu(a)))) along time.  LDS holds the depthwise taps transposed to [kernel][d] (float4 columns
// swizzled by the tap index, so the transposing stores spread over the banks and the row reads stay conflict-free) and the staged
// rows of one tile of one sample with its kernel - 1 halo rows; rows before 0 and at or after T are zero, never another sample's.
//   forward          one workgroup per 16-row tile: stages glu(a) of rows t0 - k/2 .. t0 + 15 + k/2, then one wave per row forms the
//                    taps, the LayerNorm (the statistics above) and the Swish.
//   backward role A  workgroups walk 8-row tiles: RECOMPUTE glu(a) of the tile and its halo rows, and DW, the LayerNorm statistics and
//                    the Swish argument of the tile's own rows; form dv (the gradient at the depthwise output) of the own rows, keep it in
//                    LDS and write it to the workspace; sum d(dw bias), dgamma, dbeta per lane and d(dw weight) per (tap, float4 column)
//                    thread over the tile's rows in row order; one slab per workgroup, slabs added in slab order by the finishing launch.
//   backward role B  one workgroup per 16-row tile (a second launch: dv of the halo rows belongs to other tiles): stages dv of rows
//                    t0 - k/2 .. t0 + 15 + k/2 from the workspace, forms the transposed taps and RECOMPUTES sigmoid of the gate half of
//                    the tile's own rows for the GLU's backward.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "nn_common.h"

// forward and backward must agree on every recomputed value: every fused multiply-add of this file is written as fmaf
#pragma clang fp contract(off)

namespace {

constexpr int CF_THREADS = 256, CF_WAVES = CF_THREADS / 64, CF_LN_MAX_BLOCKS = 256, CF_BSD_MAX_BLOCKS = 64;
constexpr int CV_TILE = SALSA_NN_CONV_MODULE_TILE, CV_BWD_TILE = 8, CV_BWD_MAX_BLOCKS = 128, CV_MAX_T = 512, CV_MAX_KERNEL = 31;

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ inline float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// the mask of four neighbouring elements whose first has the (even) flat index `first`
__device__ inline void drop_keep4(uint64_t first, const DropArgs &d, bool (&keep)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        const unsigned h = drop_hash((unsigned)(first >> 1) + k / 2, d.seed);
        keep[k] = (h & 0xFFFFu) >= d.thresh;
        keep[k + 1] = (h >> 16) >= d.thresh;
    }
}

// two-pass row statistics over the 64 lanes' E elements each: add_layernorm_fwd_kernel's, operation for operation
template <int E>
__device__ inline void row_stats(const float (&z)[E], float eps, float &mu, float &rs)
{
    constexpr int C = 64 * E;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) s += z[e];
    const float mu0 = wave_sum(s) * (1.f / C);
    s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) s += z[e] - mu0;
    mu = fmaf(wave_sum(s), 1.f / C, mu0);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) q = fmaf(z[e] - mu, z[e] - mu, q);
    rs = 1.f / sqrtf(wave_sum(q) * (1.f / C) + eps);
}

template <int C>
__device__ inline void load_row(const float *__restrict__ p, int64_t row, int lane, float (&v)[C / 64])
{
#pragma unroll
    for (int n = 0; n < C / 256; n++) {
        const float4 t = *reinterpret_cast<const float4 *>(p + row * C + 256 * n + 4 * lane);
        v[4 * n] = t.x, v[4 * n + 1] = t.y, v[4 * n + 2] = t.z, v[4 * n + 3] = t.w;
    }
}

template <int C>
__device__ inline void store_row(float *__restrict__ p, int64_t row, int lane, const float (&v)[C / 64])
{
#pragma unroll
    for (int n = 0; n < C / 256; n++)
        *reinterpret_cast<float4 *>(p + row * C + 256 * n + 4 * lane) = make_float4(v[4 * n], v[4 * n + 1], v[4 * n + 2], v[4 * n + 3]);
}

// ---- res_layernorm ---------------------------------------------------------------------------------------------------------------
// z = x + scale * (branch * dropscale) where the mask keeps, x where it drops; keep[] is left for the caller
template <int C>
__device__ inline void res_row(const float *__restrict__ x, const float *__restrict__ branch, float scale, const DropArgs &drop, int64_t row,
                               int lane, float (&z)[C / 64], bool (&keep)[C / 64])
{
    load_row<C>(x, row, lane, z);
#pragma unroll
    for (int e = 0; e < C / 64; e++) keep[e] = true;
    if (!branch) return;
    float r[C / 64];
    load_row<C>(branch, row, lane, r);
#pragma unroll
    for (int n = 0; n < C / 256; n++) {
        bool k4[4] = {true, true, true, true};
        if (drop.thresh) drop_keep4((uint64_t)row * C + 256 * n + 4 * lane, drop, k4);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            keep[4 * n + k] = k4[k];
            if (k4[k]) z[4 * n + k] = z[4 * n + k] + scale * (r[4 * n + k] * drop.scale);
        }
    }
}

template <int C>
__global__ __launch_bounds__(CF_THREADS) void res_ln_fwd_kernel(const float *__restrict__ x, const float *__restrict__ branch, float scale,
                                                                DropArgs drop, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float *__restrict__ z_out,
                                                                float *__restrict__ y, float *__restrict__ mean, float *__restrict__ rstd,
                                                                int64_t M, float eps)
{
    constexpr int E = C / 64;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * CF_WAVES + (threadIdx.x >> 6);
    if (row >= M) return;                                                     // (whole waves: no barrier in this kernel)
    float z[E];
    bool keep[E];
    res_row<C>(x, branch, scale, drop, row, lane, z, keep);
    if (z_out) store_row<C>(z_out, row, lane, z);
    if (!y) return;
    float mu, rs, gm[E], bt[E];
    row_stats<E>(z, eps, mu, rs);
    load_row<C>(gamma, 0, lane, gm);
    load_row<C>(beta, 0, lane, bt);
#pragma unroll
    for (int e = 0; e < E; e++) z[e] = fmaf((z[e] - mu) * rs, gm[e], bt[e]);
    store_row<C>(y, row, lane, z);
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

inline int res_ln_blocks(int64_t M)
{
    const int64_t nb = (M + CF_WAVES - 1) / CF_WAVES;
    return (int)(nb < CF_LN_MAX_BLOCKS ? nb : CF_LN_MAX_BLOCKS);
}

template <int C>
__global__ __launch_bounds__(CF_THREADS) void res_ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ dz_in,
                                                                const float *__restrict__ x, const float *__restrict__ branch, float scale,
                                                                DropArgs drop, const float *__restrict__ gamma,
                                                                const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                float *__restrict__ dx, float *__restrict__ dbranch,
                                                                float *__restrict__ ws /* [grid][2][C] */, int64_t M)
{
    constexpr int E = C / 64;
    __shared__ float part[CF_WAVES][2][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gm[E], dg[E], db[E];
#pragma unroll
    for (int e = 0; e < E; e++) gm[e] = dg[e] = db[e] = 0.f;
    if (dy) load_row<C>(gamma, 0, lane, gm);
    for (int64_t row = (int64_t)blockIdx.x * CF_WAVES + wave; row < M; row += (int64_t)gridDim.x * CF_WAVES) {
        float z[E], r[E];
        bool keep[E];
        res_row<C>(x, branch, scale, drop, row, lane, z, keep);
#pragma unroll
        for (int e = 0; e < E; e++) r[e] = 0.f;
        if (dy) {                                                             // add_layernorm_bwd_kernel's row, operation for operation
            float g[E];
            load_row<C>(dy, row, lane, g);
            const float mu = mean[row], rs = rstd[row];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < E; e++) {
                z[e] = (z[e] - mu) * rs;                                      // xhat
                dg[e] = fmaf(g[e], z[e], dg[e]);
                db[e] += g[e];
                g[e] *= gm[e];
                s1 += g[e];
                s2 = fmaf(g[e], z[e], s2);
            }
            const float m1 = wave_sum(s1) * (1.f / C), m2 = wave_sum(s2) * (1.f / C);
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = rs * (g[e] - m1 - z[e] * m2);
        }
        if (dz_in) {
            float t[E];
            load_row<C>(dz_in, row, lane, t);
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = t[e] + r[e];
        }
        store_row<C>(dx, row, lane, r);
        if (dbranch) {
#pragma unroll
            for (int e = 0; e < E; e++) r[e] = keep[e] ? scale * (r[e] * drop.scale) : 0.f;
            store_row<C>(dbranch, row, lane, r);
        }
    }
    if (!dy) return;                                                          // (uniform over the grid)
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int col = 256 * (e >> 2) + 4 * lane + (e & 3);
        part[wave][0][col] = dg[e];
        part[wave][1][col] = db[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += CF_THREADS) {                   // waves added in wave order
        float t = (&part[0][0][0])[i];
#pragma unroll
        for (int w = 1; w < CF_WAVES; w++) t += (&part[w][0][0])[i];
        ws[(int64_t)blockIdx.x * 2 * C + i] = t;
    }
}

// out[i] = sum over slabs of ws[slab][i], slabs in slab order; i < n0 goes to out0, the rest to out1 (out1 may be NULL when n == n0)
__global__ __launch_bounds__(CF_THREADS) void slab_finish_kernel(const float *__restrict__ ws, int n_slabs, int n, int n0,
                                                                 float *__restrict__ out0, float *__restrict__ out1)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x;
    if (i >= n) return;
    float t = 0.f;
    for (int s = 0; s < n_slabs; s++) t += ws[(int64_t)s * n + i];
    if (i < n0)
        out0[i] = t;
    else
        out1[i - n0] = t;
}

// ---- bias + Swish + dropout ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CF_THREADS) void bsd_fwd_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ h,
                                                             int64_t n_vec, int C, DropArgs drop)
{
    const int64_t v = (int64_t)blockIdx.x * CF_THREADS + threadIdx.x;
    if (v >= n_vec) return;
    const float4 av = *reinterpret_cast<const float4 *>(a + 4 * v);
    float t[4] = {av.x, av.y, av.z, av.w};
    if (b) {
        const float4 bv = *reinterpret_cast<const float4 *>(b + (4 * v) % C);
        t[0] += bv.x, t[1] += bv.y, t[2] += bv.z, t[3] += bv.w;
    }
    bool keep[4] = {true, true, true, true};
    if (drop.thresh) drop_keep4((uint64_t)(4 * v), drop, keep);
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = keep[k] ? (t[k] * sigmoidf_(t[k])) * drop.scale : 0.f;
    *reinterpret_cast<float4 *>(h + 4 * v) = make_float4(t[0], t[1], t[2], t[3]);
}

inline int bsd_blocks(int64_t M)
{
    const int64_t nb = (M + CF_WAVES - 1) / CF_WAVES;
    return (int)(nb < CF_BSD_MAX_BLOCKS ? nb : CF_BSD_MAX_BLOCKS);
}

// grid (row walkers, chunks of 64 float4 columns); ws [gridDim.x][C] or NULL
__global__ __launch_bounds__(CF_THREADS) void bsd_bwd_kernel(const float *__restrict__ dh, const float *__restrict__ a,
                                                             const float *__restrict__ b, float *__restrict__ da, float *__restrict__ ws,
                                                             int64_t M, int C, DropArgs drop)
{
    __shared__ float4 part[CF_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cv = C / 4, cx = (int)blockIdx.y * 64 + lane;
    const bool active = cx < cv;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (active && b) {
        const float4 t = *reinterpret_cast<const float4 *>(b + 4 * cx);
        bv[0] = t.x, bv[1] = t.y, bv[2] = t.z, bv[3] = t.w;
    }
    if (active)
        for (int64_t row = (int64_t)blockIdx.x * CF_WAVES + wave; row < M; row += (int64_t)gridDim.x * CF_WAVES) {
            const int64_t first = row * C + 4 * cx;
            const float4 av = *reinterpret_cast<const float4 *>(a + first), gv = *reinterpret_cast<const float4 *>(dh + first);
            float t[4] = {av.x + bv[0], av.y + bv[1], av.z + bv[2], av.w + bv[3]}, g[4] = {gv.x, gv.y, gv.z, gv.w};
            bool keep[4] = {true, true, true, true};
            if (drop.thresh) drop_keep4((uint64_t)first, drop, keep);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float s = sigmoidf_(t[k]);
                g[k] = keep[k] ? (g[k] * drop.scale) * (s * (1.f + t[k] * (1.f - s))) : 0.f;
                acc[k] += g[k];
            }
            *reinterpret_cast<float4 *>(da + first) = make_float4(g[0], g[1], g[2], g[3]);
        }
    if (!ws) return;                                                          // (uniform over the grid)
    part[wave][lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (wave == 0 && active) {                                                // waves added in wave order
        float4 t = part[0][lane];
#pragma unroll
        for (int w = 1; w < CF_WAVES; w++) t.x += part[w][lane].x, t.y += part[w][lane].y, t.z += part[w][lane].z, t.w += part[w][lane].w;
        *reinterpret_cast<float4 *>(ws + (int64_t)blockIdx.x * C + 4 * cx) = t;
    }
}

// ---- convolution module ----------------------------------------------------------------------------------------------------------
// tap k of float4 column c4 in the transposed filter image [K][D]: the column is swizzled by the tap, so the transposing stores of
// one channel's taps fall on eight bank groups while a wave's row read stays one contiguous permuted row
template <int D>
__device__ inline int tap_off(int k, int c4) { return k * D + ((c4 ^ k) << 2); }

template <int D>
__device__ inline void stage_taps(float *__restrict__ wT, const float *__restrict__ w /* [D][K] */, int K)
{
    for (int idx = threadIdx.x; idx < D * K; idx += CF_THREADS) {
        const int c = idx / K, k = idx - c * K;
        wT[tap_off<D>(k, c >> 2) + (c & 3)] = w[idx];
    }
}

// rows t_first .. t_first + rows - 1 of one sample -> dst [rows][D]; rows outside [0, T) are zero.  GLU: src has 2 D columns and the
// staged value is first half x sigmoid(second half); otherwise src has D columns and is copied.
template <int D, bool GLU>
__device__ inline void stage_rows(float *__restrict__ dst, const float *__restrict__ src, int t_first, int rows, int T)
{
    constexpr int C4 = D / 4, PITCH = GLU ? 2 * D : D;
    for (int idx = threadIdx.x; idx < rows * C4; idx += CF_THREADS) {
        const int r = idx / C4, c4 = idx - r * C4, t = t_first + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) {
            const float *p = src + (int64_t)t * PITCH + 4 * c4;
            v = *reinterpret_cast<const float4 *>(p);
            if (GLU) {
                const float4 gt = *reinterpret_cast<const float4 *>(p + D);
                v.x *= sigmoidf_(gt.x), v.y *= sigmoidf_(gt.y), v.z *= sigmoidf_(gt.z), v.w *= sigmoidf_(gt.w);
            }
        }
        *reinterpret_cast<float4 *>(dst + r * D + 4 * c4) = v;
    }
}

// v[c] = bias[c] + sum_j w[c][FLIP ? K - 1 - j : j] rows[j][c] for the lane's columns, taps in j order (bias NULL: 0)
template <int D, bool FLIP>
__device__ inline void tap_row(const float *__restrict__ rows, const float *__restrict__ wT, const float *__restrict__ bias, int K, int lane,
                               float (&v)[D / 64])
{
#pragma unroll
    for (int n = 0; n < D / 256; n++) {
        const int c4 = 64 * n + lane;
        float4 acc = bias ? *reinterpret_cast<const float4 *>(bias + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < K; j++) {
            const float4 wv = *reinterpret_cast<const float4 *>(wT + tap_off<D>(FLIP ? K - 1 - j : j, c4));
            const float4 gv = *reinterpret_cast<const float4 *>(rows + j * D + 4 * c4);
            acc.x = fmaf(wv.x, gv.x, acc.x);
            acc.y = fmaf(wv.y, gv.y, acc.y);
            acc.z = fmaf(wv.z, gv.z, acc.z);
            acc.w = fmaf(wv.w, gv.w, acc.w);
        }
        v[4 * n] = acc.x, v[4 * n + 1] = acc.y, v[4 * n + 2] = acc.z, v[4 * n + 3] = acc.w;
    }
}

// BWD false: the forward (src = a, out = u).  BWD true: the backward's role B (src = dv of the workspace, out = da, a for the GLU).
template <int D, bool BWD>
__global__ __launch_bounds__(CF_THREADS) void conv_tile_kernel(const float *__restrict__ src, const float *__restrict__ a,
                                                               const float *__restrict__ w, const float *__restrict__ wb,
                                                               const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               float *__restrict__ out, int T, int K, float eps)
{
    constexpr int E = D / 64;
    extern __shared__ __attribute__((aligned(16))) float cf_lds[];
    float *wT = cf_lds, *rows = cf_lds + K * D;                               // [K][D], [CV_TILE + K - 1][D]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t0 = (int)blockIdx.x * CV_TILE, b = blockIdx.y;
    stage_taps<D>(wT, w, K);
    stage_rows<D, !BWD>(rows, src + (int64_t)b * T * (BWD ? D : 2 * D), t0 - K / 2, CV_TILE + K - 1, T);
    __syncthreads();
    for (int i = wave; i < CV_TILE && t0 + i < T; i += CF_WAVES) {            // (wave-uniform)
        const int64_t row = (int64_t)b * T + t0 + i;
        float v[E];
        if (!BWD) {
            tap_row<D, false>(rows + i * D, wT, wb, K, lane, v);
            float mu, rs, gm[E], bt[E];
            row_stats<E>(v, eps, mu, rs);
            load_row<D>(gamma, 0, lane, gm);
            load_row<D>(beta, 0, lane, bt);
#pragma unroll
            for (int e = 0; e < E; e++) {
                const float y = fmaf((v[e] - mu) * rs, gm[e], bt[e]);
                v[e] = y * sigmoidf_(y);
            }
            store_row<D>(out, row, lane, v);
        } else {
            tap_row<D, true>(rows + i * D, wT, nullptr, K, lane, v);
            float a1[E], a2[E];
            load_row<D>(a, 2 * row, lane, a1);                                // (rows of 2 D: the value half is row 2 r of D columns,
            load_row<D>(a, 2 * row + 1, lane, a2);                            //  the gate half row 2 r + 1)
#pragma unroll
            for (int e = 0; e < E; e++) {
                const float s = sigmoidf_(a2[e]);
                a2[e] = (v[e] * a1[e]) * (s * (1.f - s));
                a1[e] = v[e] * s;
            }
            store_row<D>(out, 2 * row, lane, a1);
            store_row<D>(out, 2 * row + 1, lane, a2);
        }
    }
}

// the backward's role A; slab of a workgroup: [K][D] d(dw weight) transposed, then d(dw bias), dgamma, dbeta [D] each
template <int D>
__global__ __launch_bounds__(CF_THREADS) void conv_bwd_rows_kernel(const float *__restrict__ a, const float *__restrict__ du,
                                                                   const float *__restrict__ w, const float *__restrict__ wb,
                                                                   const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                   float *__restrict__ dv_ws, float *__restrict__ slab_ws, int B, int T, int K,
                                                                   float eps)
{
    constexpr int E = D / 64, C4 = D / 4, KG = CF_THREADS / C4, MAXJ = (CV_MAX_KERNEL + KG - 1) / KG;
    extern __shared__ __attribute__((aligned(16))) float cf_lds[];
    float *wT = cf_lds, *g = wT + K * D, *dvt = g + (CV_BWD_TILE + K - 1) * D;   // [K][D], [CV_BWD_TILE + K - 1][D], [CV_BWD_TILE][D]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cg = threadIdx.x % C4, kg = threadIdx.x / C4;
    const int n_tiles = (T + CV_BWD_TILE - 1) / CV_BWD_TILE, total = B * n_tiles;
    stage_taps<D>(wT, w, K);
    float gm[E], bt[E], dgam[E], dbet[E], dbias[E];
    float4 dwacc[MAXJ];
    load_row<D>(gamma, 0, lane, gm);
    load_row<D>(beta, 0, lane, bt);
#pragma unroll
    for (int e = 0; e < E; e++) dgam[e] = dbet[e] = dbias[e] = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; j++) dwacc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int b = tile / n_tiles, t0 = (tile - b * n_tiles) * CV_BWD_TILE;
        stage_rows<D, true>(g, a + (int64_t)b * T * 2 * D, t0 - K / 2, CV_BWD_TILE + K - 1, T);
        __syncthreads();
        for (int i = wave; i < CV_BWD_TILE; i += CF_WAVES) {
            float v[E];
            if (t0 + i < T) {                                                 // (wave-uniform)
                const int64_t row = (int64_t)b * T + t0 + i;
                float gu[E], mu, rs;
                tap_row<D, false>(g + i * D, wT, wb, K, lane, v);
                row_stats<E>(v, eps, mu, rs);
                load_row<D>(du, row, lane, gu);
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int e = 0; e < E; e++) {
                    v[e] = (v[e] - mu) * rs;                                  // xhat
                    const float y = fmaf(v[e], gm[e], bt[e]), s = sigmoidf_(y);
                    gu[e] *= s * (1.f + y * (1.f - s));                       // dy
                    dgam[e] = fmaf(gu[e], v[e], dgam[e]);
                    dbet[e] += gu[e];
                    gu[e] *= gm[e];
                    s1 += gu[e];
                    s2 = fmaf(gu[e], v[e], s2);
                }
                const float m1 = wave_sum(s1) * (1.f / D), m2 = wave_sum(s2) * (1.f / D);
#pragma unroll
                for (int e = 0; e < E; e++) {
                    v[e] = rs * (gu[e] - m1 - v[e] * m2);                     // dv
                    dbias[e] += v[e];
                }
                store_row<D>(dv_ws, row, lane, v);
            } else {
#pragma unroll
                for (int e = 0; e < E; e++) v[e] = 0.f;
            }
            store_row<D>(dvt, i, lane, v);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MAXJ; j++) {                                      // d(dw weight)[c][k] += sum_i dv[i][c] glu[i - K/2 + k][c]
            const int k = kg + KG * j;
            if (k < K) {
#pragma unroll
                for (int i = 0; i < CV_BWD_TILE; i++) {
                    const float4 dv = *reinterpret_cast<const float4 *>(dvt + i * D + 4 * cg);
                    const float4 gv = *reinterpret_cast<const float4 *>(g + (i + k) * D + 4 * cg);
                    dwacc[j].x = fmaf(dv.x, gv.x, dwacc[j].x);
                    dwacc[j].y = fmaf(dv.y, gv.y, dwacc[j].y);
                    dwacc[j].z = fmaf(dv.z, gv.z, dwacc[j].z);
                    dwacc[j].w = fmaf(dv.w, gv.w, dwacc[j].w);
                }
            }
        }
        __syncthreads();                                                      // the next tile overwrites g and dvt
    }
    float *slab = slab_ws + (int64_t)blockIdx.x * (K + 3) * D;
#pragma unroll
    for (int j = 0; j < MAXJ; j++) {
        const int k = kg + KG * j;
        if (k < K) *reinterpret_cast<float4 *>(slab + k * D + 4 * cg) = dwacc[j];
    }
    float *part = cf_lds;                                                     // [CF_WAVES][3][D] over the taps and rows, which are done with
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int col = 256 * (e >> 2) + 4 * lane + (e & 3);
        part[(wave * 3 + 0) * D + col] = dbias[e];
        part[(wave * 3 + 1) * D + col] = dgam[e];
        part[(wave * 3 + 2) * D + col] = dbet[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * D; i += CF_THREADS) {                   // waves added in wave order
        float t = part[i];
#pragma unroll
        for (int wv = 1; wv < CF_WAVES; wv++) t += part[wv * 3 * D + i];
        slab[K * D + i] = t;
    }
}

// slabs added in slab order -> dw [D][K] (transposed back), dbias, dgamma, dbeta [D]
__global__ __launch_bounds__(CF_THREADS) void conv_bwd_finish_kernel(const float *__restrict__ ws, int n_slabs, int D, int K,
                                                                     float *__restrict__ dw, float *__restrict__ dbias,
                                                                     float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int i = blockIdx.x * CF_THREADS + threadIdx.x, n = (K + 3) * D;
    if (i >= n) return;
    float t = 0.f;
    for (int s = 0; s < n_slabs; s++) t += ws[(int64_t)s * n + i];
    const int k = i / D, c = i - k * D;
    if (k < K)
        dw[c * K + k] = t;
    else
        (k == K ? dbias : k == K + 1 ? dgamma : dbeta)[c] = t;
}

bool rows_ok(int64_t M, int C) { return M >= 1 && (C == 256 || C == 512) && M * C < ((int64_t)1 << 32); }
bool drop_ok(float p) { return p >= 0.f && p < 1.f; }
bool bsd_ok(int64_t M, int C) { return M >= 1 && C >= 4 && C <= 4096 && C % 4 == 0 && M * C < ((int64_t)1 << 32); }
bool conv_ok(int64_t B, int T, int d, int kernel)
{
    return (d == 256 || d == 512) && T >= 1 && T <= CV_MAX_T && kernel >= 3 && kernel <= CV_MAX_KERNEL && (kernel & 1) && B >= 1 && B <= 65535;
}
int conv_bwd_blocks(int B, int T)
{
    const int64_t total = (int64_t)B * ((T + CV_BWD_TILE - 1) / CV_BWD_TILE);
    return (int)(total < CV_BWD_MAX_BLOCKS ? total : CV_BWD_MAX_BLOCKS);
}
size_t conv_fwd_lds(int d, int kernel) { return (size_t)(CV_TILE + 2 * kernel - 1) * d * sizeof(float); }
size_t conv_bwd_lds(int d, int kernel) { return (size_t)(2 * CV_BWD_TILE + 2 * kernel - 1) * d * sizeof(float); }

// a workgroup of these kernels may take more than the 64 KiB of LDS a launch gets by default: raised once per device and kernel
template <typename F>
bool allow_lds(F *kernel, int slot)
{
    static bool done[64][6] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (dev >= 0 && dev < 64 && done[dev][slot]) return true;
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;
    if (dev >= 0 && dev < 64) done[dev][slot] = true;
    return true;
}

} // namespace

extern "C" int salsa_nn_res_layernorm_supported(int64_t M, int C) { return rows_ok(M, C) ? 1 : 0; }

extern "C" size_t salsa_nn_res_layernorm_ws_bytes(int64_t M, int C)
{
    return rows_ok(M, C) ? (size_t)res_ln_blocks(M) * 2 * (size_t)C * sizeof(float) : 0;
}

extern "C" int salsa_nn_res_layernorm_fwd(const float *x, const float *branch, float scale, float drop_p, uint32_t drop_seed,
                                          const float *gamma, const float *beta, float *z_out, float *y_out, float *mean, float *rstd,
                                          int64_t M, int C, float eps, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!x || (!z_out && !y_out) || (y_out && (!gamma || !beta || !mean || !rstd))) return -1;
    if (!rows_ok(M, C) || !drop_ok(drop_p) || !(eps >= 0.f)) return -1;
    const dim3 grid((unsigned)((M + CF_WAVES - 1) / CF_WAVES));
    const DropArgs drop = drop_args(branch ? drop_p : 0.f, drop_seed);
    if (C == 256)
        hipLaunchKernelGGL(res_ln_fwd_kernel<256>, grid, dim3(CF_THREADS), 0, (hipStream_t)hip_stream, x, branch, scale, drop, gamma, beta, z_out,
                           y_out, mean, rstd, M, eps);
    else
        hipLaunchKernelGGL(res_ln_fwd_kernel<512>, grid, dim3(CF_THREADS), 0, (hipStream_t)hip_stream, x, branch, scale, drop, gamma, beta, z_out,
                           y_out, mean, rstd, M, eps);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_res_layernorm_bwd(const float *dy, const float *dz_in, const float *x, const float *branch, float scale, float drop_p,
                                          uint32_t drop_seed, const float *gamma, const float *mean, const float *rstd, float *dx,
                                          float *dbranch, float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int64_t M, int C,
                                          void *hip_stream)
{
    if (!x || !dx || (!dy && !dz_in) || (dbranch && !branch)) return -1;
    if (dy && (!gamma || !mean || !rstd || !dgamma || !dbeta || !ws)) return -1;
    if (!rows_ok(M, C) || !drop_ok(drop_p)) return -1;
    if (dy && ws_bytes < salsa_nn_res_layernorm_ws_bytes(M, C)) return -5;
    const int nb = res_ln_blocks(M);
    const DropArgs drop = drop_args(branch ? drop_p : 0.f, drop_seed);
    if (C == 256)
        hipLaunchKernelGGL(res_ln_bwd_kernel<256>, dim3(nb), dim3(CF_THREADS), 0, (hipStream_t)hip_stream, dy, dz_in, x, branch, scale, drop,
                           gamma, mean, rstd, dx, dbranch, (float *)ws, M);
    else
        hipLaunchKernelGGL(res_ln_bwd_kernel<512>, dim3(nb), dim3(CF_THREADS), 0, (hipStream_t)hip_stream, dy, dz_in, x, branch, scale, drop,
                           gamma, mean, rstd, dx, dbranch, (float *)ws, M);
    if (dy)
        hipLaunchKernelGGL(slab_finish_kernel, dim3((2 * C + CF_THREADS - 1) / CF_THREADS), dim3(CF_THREADS), 0, (hipStream_t)hip_stream,
                           (const float *)ws, nb, 2 * C, C, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_bias_swish_dropout_supported(int64_t M, int C) { return bsd_ok(M, C) ? 1 : 0; }

extern "C" size_t salsa_nn_bias_swish_dropout_ws_bytes(int64_t M, int C)
{
    return bsd_ok(M, C) ? (size_t)bsd_blocks(M) * (size_t)C * sizeof(float) : 0;
}

extern "C" int salsa_nn_bias_swish_dropout_fwd(const float *a, const float *bias, float *h, int64_t M, int C, float drop_p, uint32_t drop_seed,
                                               void *hip_stream)
{
    if (!a || !h || !bsd_ok(M, C) || !drop_ok(drop_p)) return -1;
    const int64_t n_vec = M * C / 4;
    hipLaunchKernelGGL(bsd_fwd_kernel, dim3((unsigned)((n_vec + CF_THREADS - 1) / CF_THREADS)), dim3(CF_THREADS), 0, (hipStream_t)hip_stream, a,
                       bias, h, n_vec, C, drop_args(drop_p, drop_seed));
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_bias_swish_dropout_bwd(const float *dh, const float *a, const float *bias, float *da, float *dbias, void *ws,
                                               size_t ws_bytes, int64_t M, int C, float drop_p, uint32_t drop_seed, void *hip_stream)
{
    if (!dh || !a || !da || (dbias && !ws) || !bsd_ok(M, C) || !drop_ok(drop_p)) return -1;
    if (dbias && ws_bytes < salsa_nn_bias_swish_dropout_ws_bytes(M, C)) return -5;
    const int nb = bsd_blocks(M);
    hipLaunchKernelGGL(bsd_bwd_kernel, dim3(nb, (C / 4 + 63) / 64), dim3(CF_THREADS), 0, (hipStream_t)hip_stream, dh, a, bias, da,
                       dbias ? (float *)ws : nullptr, M, C, drop_args(drop_p, drop_seed));
    if (dbias)
        hipLaunchKernelGGL(slab_finish_kernel, dim3((C + CF_THREADS - 1) / CF_THREADS), dim3(CF_THREADS), 0, (hipStream_t)hip_stream,
                           (const float *)ws, nb, C, C, dbias, (float *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_conv_module_supported(int T, int d, int kernel) { return conv_ok(1, T, d, kernel) ? 1 : 0; }

extern "C" size_t salsa_nn_conv_module_ws_bytes(int B, int T, int d, int kernel)
{
    if (!conv_ok(B, T, d, kernel)) return 0;
    return ((size_t)B * T * d + (size_t)conv_bwd_blocks(B, T) * (kernel + 3) * d) * sizeof(float);
}

extern "C" int salsa_nn_conv_module_fwd(const float *a, const float *dw_weight, const float *dw_bias, const float *gamma, const float *beta,
                                        float *u, int B, int T, int d, int kernel, float eps, void *hip_stream)
{
    if (!a || !dw_weight || !dw_bias || !gamma || !beta || !u || !conv_ok(B, T, d, kernel) || !(eps >= 0.f)) return -1;
    const dim3 grid((unsigned)((T + CV_TILE - 1) / CV_TILE), (unsigned)B);
    const size_t lds = conv_fwd_lds(d, kernel);
    if (d == 256) {
        if (!allow_lds(conv_tile_kernel<256, false>, 0)) return -6;
        hipLaunchKernelGGL((conv_tile_kernel<256, false>), grid, dim3(CF_THREADS), lds, (hipStream_t)hip_stream, a, a, dw_weight, dw_bias, gamma,
                           beta, u, T, kernel, eps);
    } else {
        if (!allow_lds(conv_tile_kernel<512, false>, 1)) return -6;
        hipLaunchKernelGGL((conv_tile_kernel<512, false>), grid, dim3(CF_THREADS), lds, (hipStream_t)hip_stream, a, a, dw_weight, dw_bias, gamma,
                           beta, u, T, kernel, eps);
    }
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_conv_module_bwd(const float *du, const float *a, const float *dw_weight, const float *dw_bias, const float *gamma,
                                        const float *beta, float *da, float *d_dw_weight, float *d_dw_bias, float *dgamma, float *dbeta,
                                        void *ws, size_t ws_bytes, int B, int T, int d, int kernel, float eps, void *hip_stream)
{
    if (!du || !a || !dw_weight || !dw_bias || !gamma || !beta || !da || !d_dw_weight || !d_dw_bias || !dgamma || !dbeta || !ws) return -1;
    if (!conv_ok(B, T, d, kernel) || !(eps >= 0.f)) return -1;
    if (ws_bytes < salsa_nn_conv_module_ws_bytes(B, T, d, kernel)) return -5;
    hipStream_t st = (hipStream_t)hip_stream;
    float *dv = (float *)ws, *slabs = dv + (size_t)B * T * d;
    const int nb = conv_bwd_blocks(B, T);
    const dim3 grid((unsigned)((T + CV_TILE - 1) / CV_TILE), (unsigned)B);
    const size_t lds_a = conv_bwd_lds(d, kernel), lds_b = conv_fwd_lds(d, kernel);
    if (d == 256) {
        if (!allow_lds(conv_bwd_rows_kernel<256>, 2) || !allow_lds(conv_tile_kernel<256, true>, 3)) return -6;
        hipLaunchKernelGGL(conv_bwd_rows_kernel<256>, dim3(nb), dim3(CF_THREADS), lds_a, st, a, du, dw_weight, dw_bias, gamma, beta, dv, slabs,
                           B, T, kernel, eps);
        hipLaunchKernelGGL((conv_tile_kernel<256, true>), grid, dim3(CF_THREADS), lds_b, st, (const float *)dv, a, dw_weight, dw_bias, gamma,
                           beta, da, T, kernel, eps);
    } else {
        if (!allow_lds(conv_bwd_rows_kernel<512>, 4) || !allow_lds(conv_tile_kernel<512, true>, 5)) return -6;
        hipLaunchKernelGGL(conv_bwd_rows_kernel<512>, dim3(nb), dim3(CF_THREADS), lds_a, st, a, du, dw_weight, dw_bias, gamma, beta, dv, slabs,
                           B, T, kernel, eps);
        hipLaunchKernelGGL((conv_tile_kernel<512, true>), grid, dim3(CF_THREADS), lds_b, st, (const float *)dv, a, dw_weight, dw_bias, gamma,
                           beta, da, T, kernel, eps);
    }
    const int n = (kernel + 3) * d;
    hipLaunchKernelGGL(conv_bwd_finish_kernel, dim3((n + CF_THREADS - 1) / CF_THREADS), dim3(CF_THREADS), 0, st, (const float *)slabs, nb, d,
                       kernel, d_dw_weight, d_dw_bias, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
