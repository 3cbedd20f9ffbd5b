// attention.hip -- the decoder's optional self-attention stage (include/salsa_nn.h): the attention core
// softmax(Q K^T / sqrt(dh)) V with its backward, and the fused residual add + LayerNorm with its backward.  All float32, plain FMAs
// (products exact in float32, float32 accumulation): the stage is a few GFLOP per pass and latency-bound, not rate-bound.
//
// Attention core.  qkv is (B, T, 3, heads, dh), the in-projection's output as it is; out is (B, T, heads * dh); lse (B, heads, T).
// Every product is a 64 x 64 tile computed by a workgroup of 256 threads as a 16 x 16 grid: thread (ty, tx) owns rows ty + 16 a and
// columns tx + 16 c (a, c = 0 .. 3), so the 16 lanes of a ds_read_b128 group read 16 rows whose starts are 4 banks apart (row pitch
// dh + 4 floats): conflict-free.  Two product forms cover everything:
//   nt   acc[a][c] += sum_k A[row a][k] B[row c][k]        (both operands read along their rows: Q K^T, dO V^T, K Q^T, V dO^T)
//   nn   acc[a][c'] += sum_k A[row a][k] B[k][col c']      (A is a 64 x 64 probability / dS tile in LDS, B an operand tile: P V, dS K, ...)
// Forward: one workgroup per (query tile, head, sample) walks the key tiles with an online softmax (running row maximum and sum; the
// output tile is rescaled in registers) -- it owns all keys of its rows.  Backward: ONE launch with two roles.  Role 0, one
// workgroup per query tile, walks the key tiles and owns dQ of its rows; role 1, one workgroup per key tile, walks the query tiles
// with the transposed tiles (S^T = K Q^T, dP^T = V dO^T) and owns dK and dV of its keys.  P is recomputed from lse (never stored)
// and no result is summed across workgroups: no atomics, fixed summation order, so both passes are bit-reproducible and a sample's
// result does not depend on the rest of the batch.  dP - delta (delta_i = dO_i . o_i) is ONE sum, D_ij = sum_d dO_id (v_jd - o_id):
// no delta pass, no row constant to preload, and its rounding error scales with |v_j - o_i| -- zero where one key holds the row,
// where the difference of two finished sums leaves rounding noise of the size of |dO_i . v_j| in dS.  The logits are rounded after
// the scale in both passes, so exp(S - lse) sees the forward's own S.
// Rows past T are zero-filled in LDS and their probabilities forced to zero.
//
// Add + LayerNorm.  One wave per row (C = 256 or 512: one or two float4 per lane), two-pass statistics (the mean with one correction
// step, mu0 + mean(z - mu0), then the mean of squared deviations), butterfly wave reductions.  Backward: the same row-per-wave walk
// over a fixed grid; every lane keeps the dgamma / dbeta partial sums of its columns, the four waves of a workgroup are added in wave
// order into the workgroup's slab of the workspace, and a second launch adds the slabs in slab order: bit-reproducible for a given M.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"

// every fused multiply-add of this file is written as fmaf: a product the compiler fuses on its own in one pass and not in the other
// (the scaled logit in exp(S - lse)) would break the bit-for-bit agreement the backward relies on
#pragma clang fp contract(off)

namespace {

constexpr int ATT_THREADS = 256, ATT_TILE = 64, ATT_PLD = ATT_TILE + 4, ATT_MAX_T = 512;

// a 64-row tile of one head's operand: rows t0 .. t0 + 63 of `src` (row pitch `pitch` floats, DH floats used) -> LDS [64][DH + 4];
// rows at or past T are zero
template <int DH>
__device__ inline void load_tile(float *__restrict__ dst, const float *__restrict__ src, int64_t pitch, int t0, int T)
{
    constexpr int LD = DH + 4, C4 = DH / 4;
#pragma unroll
    for (int n = 0; n < ATT_TILE * C4 / ATT_THREADS; n++) {
        const int idx = (int)threadIdx.x + ATT_THREADS * n;
        const int row = idx / C4, c4 = idx - row * C4, t = t0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < T) v = *reinterpret_cast<const float4 *>(src + (int64_t)t * pitch + 4 * c4);
        *reinterpret_cast<float4 *>(dst + row * LD + 4 * c4) = v;
    }
}

// one step of every dot product over the head dimension: four fused multiply-adds into the running sum, in k order (a plain k-ordered
// chain, what a float32 GEMM does per output element; dot4_step is the ONLY form used, so equal operands give equal bits everywhere)
__device__ inline float dot4_step(const float4 a, const float4 b, float acc)
{
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

// acc[a][c] += sum_k A[(ty + 16 a)][k] B[(tx + 16 c)][k], by dot4_step in k order
template <int K, int LDA, int LDB>
__device__ inline void mm_nt(const float *__restrict__ A, const float *__restrict__ B, int ty, int tx, float (&acc)[4][4])
{
#pragma unroll 4
    for (int k = 0; k < K; k += 4) {
        float4 av[4], bv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) av[a] = *reinterpret_cast<const float4 *>(A + (ty + 16 * a) * LDA + k);
#pragma unroll
        for (int c = 0; c < 4; c++) bv[c] = *reinterpret_cast<const float4 *>(B + (tx + 16 * c) * LDB + k);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[a][c] = dot4_step(av[a], bv[c], acc[a][c]);
    }
}

// the backward's dP - delta in one sum: acc[a][c] += sum_k G[query][k] (V[key][k] - O[query][k]), the query on the tile's rows
// (QUERY_ON_ROWS: query = ty + 16 a, key = tx + 16 c) or on its columns (query = tx + 16 c, key = ty + 16 a).  Mathematically
// dO_i . v_j - dO_i . o_i; summed as differences its rounding error scales with |v_j - o_i|, which vanishes where one key holds the
// row, instead of with |dO_i . v_j| as the difference of two finished sums does (and no delta pass is needed).
template <int K, int LD, bool QUERY_ON_ROWS>
__device__ inline void mm_nt_diff(const float *__restrict__ G, const float *__restrict__ V, const float *__restrict__ O, int ty, int tx,
                                  float (&acc)[4][4])
{
    const int rq = QUERY_ON_ROWS ? ty : tx, rk = QUERY_ON_ROWS ? tx : ty;
#pragma unroll 2
    for (int k = 0; k < K; k += 4) {
        float4 gv[4], ov[4], vv[4];
#pragma unroll
        for (int n = 0; n < 4; n++) {
            gv[n] = *reinterpret_cast<const float4 *>(G + (rq + 16 * n) * LD + k);
            ov[n] = *reinterpret_cast<const float4 *>(O + (rq + 16 * n) * LD + k);
            vv[n] = *reinterpret_cast<const float4 *>(V + (rk + 16 * n) * LD + k);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int nq = QUERY_ON_ROWS ? a : c, nk = QUERY_ON_ROWS ? c : a;
                acc[a][c] = fmaf(gv[nq].x, vv[nk].x - ov[nq].x, acc[a][c]);
                acc[a][c] = fmaf(gv[nq].y, vv[nk].y - ov[nq].y, acc[a][c]);
                acc[a][c] = fmaf(gv[nq].z, vv[nk].z - ov[nq].z, acc[a][c]);
                acc[a][c] = fmaf(gv[nq].w, vv[nk].w - ov[nq].w, acc[a][c]);
            }
    }
}

// acc[a][c] += sum_k P[(ty + 16 a)][k] B[k][tx * CPT + c], k = 0 .. 63 in k order; P has pitch ATT_PLD, B pitch CPT * 16 + 4
template <int CPT>
__device__ inline void mm_nn(const float *__restrict__ P, const float *__restrict__ B, int ty, int tx, float (&acc)[4][CPT])
{
    constexpr int LDB = CPT * 16 + 4;
#pragma unroll 2
    for (int k = 0; k < ATT_TILE; k += 4) {
        float4 pv[4];
#pragma unroll
        for (int a = 0; a < 4; a++) pv[a] = *reinterpret_cast<const float4 *>(P + (ty + 16 * a) * ATT_PLD + k);
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            float bv[CPT];
            if constexpr (CPT == 4) {
                const float4 t = *reinterpret_cast<const float4 *>(B + (k + kk) * LDB + tx * 4);
                bv[0] = t.x, bv[1] = t.y, bv[2] = t.z, bv[3] = t.w;
            } else {
                const float2 t = *reinterpret_cast<const float2 *>(B + (k + kk) * LDB + tx * 2);
                bv[0] = t.x, bv[1] = t.y;
            }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const float p = kk == 0 ? pv[a].x : kk == 1 ? pv[a].y : kk == 2 ? pv[a].z : pv[a].w;
#pragma unroll
                for (int c = 0; c < CPT; c++) acc[a][c] = fmaf(p, bv[c], acc[a][c]);
            }
        }
    }
}

// the 16 lanes that share ty (one row group) are contiguous in the wave: butterflies over 1, 2, 4, 8 stay inside them
__device__ inline float row_max16(float v)
{
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ inline float row_sum16(float v)
{
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

template <int DH>
__global__ __launch_bounds__(ATT_THREADS) void attn_fwd_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                               float *__restrict__ lse, int T, int H, float scale)
{
    constexpr int LD = DH + 4, CPT = DH / 16;
    __shared__ __attribute__((aligned(16))) float sQ[ATT_TILE * LD], sK[ATT_TILE * LD], sV[ATT_TILE * LD], sP[ATT_TILE * ATT_PLD];
    const int i0 = blockIdx.x * ATT_TILE, h = blockIdx.y, b = blockIdx.z;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int64_t pitch = (int64_t)3 * H * DH;
    const float *q = qkv + (int64_t)b * T * pitch + (int64_t)h * DH, *k = q + (int64_t)H * DH, *v = k + (int64_t)H * DH;
    load_tile<DH>(sQ, q, pitch, i0, T);
    float o[4][CPT], m[4], l[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        m[a] = -INFINITY;
        l[a] = 0.f;
#pragma unroll
        for (int c = 0; c < CPT; c++) o[a][c] = 0.f;
    }
    for (int j0 = 0; j0 < T; j0 += ATT_TILE) {
        load_tile<DH>(sK, k, pitch, j0, T);
        load_tile<DH>(sV, v, pitch, j0, T);
        __syncthreads();
        float s[4][4];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) s[a][c] = 0.f;
        mm_nt<DH, LD, LD>(sQ, sK, ty, tx, s);
#pragma unroll
        for (int a = 0; a < 4; a++) {
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                s[a][c] = (j0 + tx + 16 * c < T) ? __fmul_rn(s[a][c], scale) : -INFINITY;   // (rounded: the backward forms the same number)
                mx = fmaxf(mx, s[a][c]);
            }
            mx = row_max16(mx);                               // finite: every key tile holds at least key j0 < T
            const float m_new = fmaxf(m[a], mx);
            const float alpha = expf(m[a] - m_new);           // the first tile: exp(-inf) = 0
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const float p = expf(s[a][c] - m_new);        // masked keys: exp(-inf) = 0
                sP[(ty + 16 * a) * ATT_PLD + tx + 16 * c] = p;
                sum += p;
            }
            sum = row_sum16(sum);
            l[a] = fmaf(l[a], alpha, sum);
            m[a] = m_new;
#pragma unroll
            for (int c = 0; c < CPT; c++) o[a][c] *= alpha;
        }
        __syncthreads();
        mm_nn<CPT>(sP, sV, ty, tx, o);
        __syncthreads();                                      // the next tile overwrites sK, sV and sP
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty + 16 * a;
        if (i >= T) continue;
        const float inv = 1.f / l[a];
        float *dst = out + ((int64_t)b * T + i) * H * DH + (int64_t)h * DH + tx * CPT;
#pragma unroll
        for (int c = 0; c < CPT; c++) dst[c] = o[a][c] * inv;
        if (tx == 0) lse[((int64_t)b * H + h) * T + i] = m[a] + logf(l[a]);
    }
}

template <int DH>
__global__ __launch_bounds__(ATT_THREADS) void attn_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ out,
                                                               const float *__restrict__ lse, const float *__restrict__ d_out,
                                                               float *__restrict__ d_qkv, int T, int H, float scale)
{
    constexpr int LD = DH + 4, CPT = DH / 16;
    // own: the tile this workgroup owns (role 0: Q and dO of its queries; role 1: K and V of its keys); walk: the tiles it walks
    __shared__ __attribute__((aligned(16))) float sOwnA[ATT_TILE * LD], sOwnB[ATT_TILE * LD], sWalkA[ATT_TILE * LD], sWalkB[ATT_TILE * LD];
    __shared__ __attribute__((aligned(16))) float sO[ATT_TILE * LD];          // the O tile of the queries (own in role 0, walked in role 1)
    __shared__ __attribute__((aligned(16))) float sP[ATT_TILE * ATT_PLD], sDS[ATT_TILE * ATT_PLD];
    __shared__ float sLse[ATT_TILE];
    const int n_tiles = (T + ATT_TILE - 1) / ATT_TILE;
    const int role = (int)blockIdx.x / n_tiles, own0 = ((int)blockIdx.x - role * n_tiles) * ATT_TILE, h = blockIdx.y, b = blockIdx.z;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    const int64_t pitch = (int64_t)3 * H * DH, opitch = (int64_t)H * DH;
    const float *q = qkv + (int64_t)b * T * pitch + (int64_t)h * DH, *k = q + opitch, *v = k + opitch;
    const float *o = out + (int64_t)b * T * opitch + (int64_t)h * DH, *g = d_out + (int64_t)b * T * opitch + (int64_t)h * DH;
    const float *lse_bh = lse + ((int64_t)b * H + h) * T;
    float *dq = d_qkv + (int64_t)b * T * pitch + (int64_t)h * DH, *dk = dq + opitch, *dv = dk + opitch;

    if (role == 0) {
        // dQ of queries own0 ..: S = Q K^T, D = dO (V - O)^T, dS = P D, dQ += dS K
        load_tile<DH>(sOwnA, q, pitch, own0, T);
        load_tile<DH>(sOwnB, g, opitch, own0, T);
        load_tile<DH>(sO, o, opitch, own0, T);
        if (threadIdx.x < ATT_TILE) sLse[threadIdx.x] = own0 + (int)threadIdx.x < T ? lse_bh[own0 + threadIdx.x] : 0.f;
        float acc[4][CPT];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < CPT; c++) acc[a][c] = 0.f;
        for (int j0 = 0; j0 < T; j0 += ATT_TILE) {
            load_tile<DH>(sWalkA, k, pitch, j0, T);
            load_tile<DH>(sWalkB, v, pitch, j0, T);
            __syncthreads();
            float s[4][4], dp[4][4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) s[a][c] = dp[a][c] = 0.f;
            mm_nt<DH, LD, LD>(sOwnA, sWalkA, ty, tx, s);
            mm_nt_diff<DH, LD, true>(sOwnB, sWalkB, sO, ty, tx, dp);
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float p = (j0 + tx + 16 * c < T) ? expf(__fmul_rn(s[a][c], scale) - sLse[ty + 16 * a]) : 0.f;
                    sDS[(ty + 16 * a) * ATT_PLD + tx + 16 * c] = p * dp[a][c];
                }
            __syncthreads();
            mm_nn<CPT>(sDS, sWalkA, ty, tx, acc);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int i = own0 + ty + 16 * a;
            if (i >= T) continue;
#pragma unroll
            for (int c = 0; c < CPT; c++) dq[(int64_t)i * pitch + tx * CPT + c] = acc[a][c] * scale;
        }
    } else {
        // dK, dV of keys own0 ..: the transposed tiles, key on the row: S^T = K Q^T, D^T = (V - O) dO^T, dV += P^T dO, dK += dS^T Q
        load_tile<DH>(sOwnA, k, pitch, own0, T);
        load_tile<DH>(sOwnB, v, pitch, own0, T);
        float acc_k[4][CPT], acc_v[4][CPT];
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < CPT; c++) acc_k[a][c] = acc_v[a][c] = 0.f;
        for (int i0 = 0; i0 < T; i0 += ATT_TILE) {
            load_tile<DH>(sWalkA, q, pitch, i0, T);
            load_tile<DH>(sWalkB, g, opitch, i0, T);
            load_tile<DH>(sO, o, opitch, i0, T);
            if (threadIdx.x < ATT_TILE) sLse[threadIdx.x] = i0 + (int)threadIdx.x < T ? lse_bh[i0 + threadIdx.x] : 0.f;
            __syncthreads();
            float s[4][4], dp[4][4];
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) s[a][c] = dp[a][c] = 0.f;
            mm_nt<DH, LD, LD>(sOwnA, sWalkA, ty, tx, s);
            mm_nt_diff<DH, LD, false>(sWalkB, sOwnB, sO, ty, tx, dp);
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float p = (i0 + tx + 16 * c < T) ? expf(__fmul_rn(s[a][c], scale) - sLse[tx + 16 * c]) : 0.f;
                    sP[(ty + 16 * a) * ATT_PLD + tx + 16 * c] = p;
                    sDS[(ty + 16 * a) * ATT_PLD + tx + 16 * c] = p * dp[a][c];
                }
            __syncthreads();
            mm_nn<CPT>(sP, sWalkB, ty, tx, acc_v);
            mm_nn<CPT>(sDS, sWalkA, ty, tx, acc_k);
            __syncthreads();
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int j = own0 + ty + 16 * a;
            if (j >= T) continue;
#pragma unroll
            for (int c = 0; c < CPT; c++) {
                dk[(int64_t)j * pitch + tx * CPT + c] = acc_k[a][c] * scale;
                dv[(int64_t)j * pitch + tx * CPT + c] = acc_v[a][c];
            }
        }
    }
}

// ---- residual add + LayerNorm ----------------------------------------------------------------------------------------------------
constexpr int LN_THREADS = 256, LN_WAVES = LN_THREADS / 64, LN_MAX_BLOCKS = 256;

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// lane's elements of a row: float4 n covers columns 256 n + 4 lane .. + 3
template <int C>
__device__ inline void ln_load_sum(const float *__restrict__ x, const float *__restrict__ res, int64_t row, int lane, float (&z)[C / 64])
{
#pragma unroll
    for (int n = 0; n < C / 256; n++) {
        const float4 a = *reinterpret_cast<const float4 *>(x + row * C + 256 * n + 4 * lane);
        const float4 r = *reinterpret_cast<const float4 *>(res + row * C + 256 * n + 4 * lane);
        z[4 * n] = a.x + r.x;
        z[4 * n + 1] = a.y + r.y;
        z[4 * n + 2] = a.z + r.z;
        z[4 * n + 3] = a.w + r.w;
    }
}

template <int C>
__global__ __launch_bounds__(LN_THREADS) void add_layernorm_fwd_kernel(const float *__restrict__ x, const float *__restrict__ res,
                                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                       float *__restrict__ y, float *__restrict__ mean,
                                                                       float *__restrict__ rstd, int64_t M, float eps)
{
    constexpr int E = C / 64;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    if (row >= M) return;                                                     // (whole waves: no barrier in this kernel)
    float z[E];
    ln_load_sum<C>(x, res, row, lane, z);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) s += z[e];
    const float mu0 = wave_sum(s) * (1.f / C);
    s = 0.f;                                                                  // one correction step: the mean of the residuals, which are
#pragma unroll                                                                // small -- a constant row ends on its value exactly
    for (int e = 0; e < E; e++) s += z[e] - mu0;
    const float mu = fmaf(wave_sum(s), 1.f / C, mu0);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) q = fmaf(z[e] - mu, z[e] - mu, q);
    const float rs = 1.f / sqrtf(wave_sum(q) * (1.f / C) + eps);
#pragma unroll
    for (int n = 0; n < C / 256; n++) {
        const float4 gm = *reinterpret_cast<const float4 *>(gamma + 256 * n + 4 * lane);
        const float4 bt = *reinterpret_cast<const float4 *>(beta + 256 * n + 4 * lane);
        float4 r;
        r.x = fmaf((z[4 * n] - mu) * rs, gm.x, bt.x);
        r.y = fmaf((z[4 * n + 1] - mu) * rs, gm.y, bt.y);
        r.z = fmaf((z[4 * n + 2] - mu) * rs, gm.z, bt.z);
        r.w = fmaf((z[4 * n + 3] - mu) * rs, gm.w, bt.w);
        *reinterpret_cast<float4 *>(y + row * C + 256 * n + 4 * lane) = r;
    }
    if (lane == 0) {
        mean[row] = mu;
        rstd[row] = rs;
    }
}

inline int ln_blocks(int64_t M)
{
    const int64_t nb = (M + LN_WAVES - 1) / LN_WAVES;
    return (int)(nb < LN_MAX_BLOCKS ? nb : LN_MAX_BLOCKS);
}

template <int C>
__global__ __launch_bounds__(LN_THREADS) void add_layernorm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                       const float *__restrict__ res, const float *__restrict__ gamma,
                                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                       float *__restrict__ dx, float *__restrict__ ws /* [grid][2][C] */,
                                                                       int64_t M)
{
    constexpr int E = C / 64;
    __shared__ float part[LN_WAVES][2][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gm[E], dg[E], db[E];
#pragma unroll
    for (int n = 0; n < C / 256; n++) {
        const float4 t = *reinterpret_cast<const float4 *>(gamma + 256 * n + 4 * lane);
        gm[4 * n] = t.x, gm[4 * n + 1] = t.y, gm[4 * n + 2] = t.z, gm[4 * n + 3] = t.w;
    }
#pragma unroll
    for (int e = 0; e < E; e++) dg[e] = db[e] = 0.f;
    for (int64_t row = (int64_t)blockIdx.x * LN_WAVES + wave; row < M; row += (int64_t)gridDim.x * LN_WAVES) {
        float z[E], g[E];
        ln_load_sum<C>(x, res, row, lane, z);
#pragma unroll
        for (int n = 0; n < C / 256; n++) {
            const float4 t = *reinterpret_cast<const float4 *>(dy + row * C + 256 * n + 4 * lane);
            g[4 * n] = t.x, g[4 * n + 1] = t.y, g[4 * n + 2] = t.z, g[4 * n + 3] = t.w;
        }
        const float mu = mean[row], rs = rstd[row];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < E; e++) {
            z[e] = (z[e] - mu) * rs;                                          // xhat
            dg[e] = fmaf(g[e], z[e], dg[e]);
            db[e] += g[e];
            g[e] *= gm[e];
            s1 += g[e];
            s2 = fmaf(g[e], z[e], s2);
        }
        const float m1 = wave_sum(s1) * (1.f / C), m2 = wave_sum(s2) * (1.f / C);
#pragma unroll
        for (int n = 0; n < C / 256; n++) {
            float4 r;
            r.x = rs * (g[4 * n] - m1 - z[4 * n] * m2);
            r.y = rs * (g[4 * n + 1] - m1 - z[4 * n + 1] * m2);
            r.z = rs * (g[4 * n + 2] - m1 - z[4 * n + 2] * m2);
            r.w = rs * (g[4 * n + 3] - m1 - z[4 * n + 3] * m2);
            *reinterpret_cast<float4 *>(dx + row * C + 256 * n + 4 * lane) = r;
        }
    }
#pragma unroll
    for (int e = 0; e < E; e++) {
        const int col = 256 * (e >> 2) + 4 * lane + (e & 3);
        part[wave][0][col] = dg[e];
        part[wave][1][col] = db[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += LN_THREADS) {                   // waves added in wave order
        float t = (&part[0][0][0])[i];
#pragma unroll
        for (int w = 1; w < LN_WAVES; w++) t += (&part[w][0][0])[i];
        ws[(int64_t)blockIdx.x * 2 * C + i] = t;
    }
}

__global__ __launch_bounds__(LN_THREADS) void add_layernorm_bwd_finish_kernel(const float *__restrict__ ws, int n_slabs, int C,
                                                                              float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    const int i = blockIdx.x * LN_THREADS + threadIdx.x;
    if (i >= 2 * C) return;
    float t = 0.f;
    for (int s = 0; s < n_slabs; s++) t += ws[(int64_t)s * 2 * C + i];        // slabs added in slab order
    if (i < C)
        dgamma[i] = t;
    else
        dbeta[i - C] = t;
}

bool attn_shape_ok(int64_t B, int T, int n_heads, int head_dim)
{
    return (head_dim == 32 || head_dim == 64) && n_heads >= 1 && n_heads <= 65535 && T >= 1 && T <= ATT_MAX_T && B >= 1 && B <= 65535;
}

} // namespace

extern "C" int salsa_nn_attn_supported(int T, int n_heads, int head_dim) { return attn_shape_ok(1, T, n_heads, head_dim) ? 1 : 0; }

extern "C" int salsa_nn_attn_fwd(const float *qkv, float *out, float *lse, int B, int T, int n_heads, int head_dim, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!qkv || !out || !lse || !attn_shape_ok(B, T, n_heads, head_dim)) return -1;
    const dim3 grid((unsigned)((T + ATT_TILE - 1) / ATT_TILE), (unsigned)n_heads, (unsigned)B);
    const float scale = (float)(1.0 / sqrt((double)head_dim));
    if (head_dim == 64)
        hipLaunchKernelGGL(attn_fwd_kernel<64>, grid, dim3(ATT_THREADS), 0, (hipStream_t)hip_stream, qkv, out, lse, T, n_heads, scale);
    else
        hipLaunchKernelGGL(attn_fwd_kernel<32>, grid, dim3(ATT_THREADS), 0, (hipStream_t)hip_stream, qkv, out, lse, T, n_heads, scale);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_attn_bwd(const float *qkv, const float *out, const float *lse, const float *d_out, float *d_qkv, int B, int T,
                                 int n_heads, int head_dim, void *hip_stream)
{
    if (!qkv || !out || !lse || !d_out || !d_qkv || !attn_shape_ok(B, T, n_heads, head_dim)) return -1;
    const dim3 grid((unsigned)(2 * ((T + ATT_TILE - 1) / ATT_TILE)), (unsigned)n_heads, (unsigned)B);   // role 0: dQ tiles, role 1: dK / dV tiles
    const float scale = (float)(1.0 / sqrt((double)head_dim));
    if (head_dim == 64)
        hipLaunchKernelGGL(attn_bwd_kernel<64>, grid, dim3(ATT_THREADS), 0, (hipStream_t)hip_stream, qkv, out, lse, d_out, d_qkv, T,
                           n_heads, scale);
    else
        hipLaunchKernelGGL(attn_bwd_kernel<32>, grid, dim3(ATT_THREADS), 0, (hipStream_t)hip_stream, qkv, out, lse, d_out, d_qkv, T,
                           n_heads, scale);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" size_t salsa_nn_add_layernorm_ws_bytes(int64_t M, int C)
{
    if (M < 1 || (C != 256 && C != 512)) return 0;
    return (size_t)ln_blocks(M) * 2 * (size_t)C * sizeof(float);
}

extern "C" int salsa_nn_add_layernorm_fwd(const float *x, const float *res, const float *gamma, const float *beta, float *y, float *mean,
                                          float *rstd, int64_t M, int C, float eps, void *hip_stream)
{
    if (!x || !res || !gamma || !beta || !y || !mean || !rstd) return -1;
    if (M < 1 || M > ((int64_t)1 << 31) - 1 || (C != 256 && C != 512) || !(eps >= 0.f)) return -1;
    const dim3 grid((unsigned)((M + LN_WAVES - 1) / LN_WAVES));
    if (C == 256)
        hipLaunchKernelGGL(add_layernorm_fwd_kernel<256>, grid, dim3(LN_THREADS), 0, (hipStream_t)hip_stream, x, res, gamma, beta, y, mean,
                           rstd, M, eps);
    else
        hipLaunchKernelGGL(add_layernorm_fwd_kernel<512>, grid, dim3(LN_THREADS), 0, (hipStream_t)hip_stream, x, res, gamma, beta, y, mean,
                           rstd, M, eps);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

extern "C" int salsa_nn_add_layernorm_bwd(const float *dy, const float *x, const float *res, const float *gamma, const float *mean,
                                          const float *rstd, float *dx, float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int64_t M,
                                          int C, void *hip_stream)
{
    if (!dy || !x || !res || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta || !ws) return -1;
    if (M < 1 || M > ((int64_t)1 << 31) - 1 || (C != 256 && C != 512)) return -1;
    if (ws_bytes < salsa_nn_add_layernorm_ws_bytes(M, C)) return -5;
    const int nb = ln_blocks(M);
    if (C == 256)
        hipLaunchKernelGGL(add_layernorm_bwd_kernel<256>, dim3(nb), dim3(LN_THREADS), 0, (hipStream_t)hip_stream, dy, x, res, gamma, mean,
                           rstd, dx, (float *)ws, M);
    else
        hipLaunchKernelGGL(add_layernorm_bwd_kernel<512>, dim3(nb), dim3(LN_THREADS), 0, (hipStream_t)hip_stream, dy, x, res, gamma, mean,
                           rstd, dx, (float *)ws, M);
    hipLaunchKernelGGL(add_layernorm_bwd_finish_kernel, dim3((2 * C + LN_THREADS - 1) / LN_THREADS), dim3(LN_THREADS), 0,
                       (hipStream_t)hip_stream, (const float *)ws, nb, C, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
