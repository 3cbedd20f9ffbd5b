// conv_c64_wrw.hip -- weight gradient of the 3x3 / 64 -> 64 convolution (conv_mfma.hip), channels-last bf16, on the gfx950 matrix
// cores through transposing LDS reads; also with the BatchNorm + ReLU + dropout in front of the layer applied while staging.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nn_det.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------------------------ weight gradient
// dW[co][tap][ci] = sum over pixels p of dy[p][co] * x[p + tap][ci]: a GEMM whose reduction runs over PIXELS, so both MFMA
// operands need 8 consecutive pixels of ONE channel per lane while memory (and the LDS tiles) are pixel-major.  gfx950's
// transposing LDS read does exactly that: ds_read_b64_tr_b16 with source lane i of a 16-lane group pointing at 4
// consecutive channels of pixel row i/4 (channel block i%4) returns to lane l channel l%16 of those 4 pixel rows
// (tools/probes/ds_tr_probe.hip prints the mapping), so two reads build one operand fragment: A = dy^T (32 co x 16 pixels),
// B = x (16 pixels x 32 ci).  A persistent workgroup keeps 64 x 576 float32 partial sums in registers (wave = one co half
// x one ci half x 9 taps = 9 accumulator tiles) over all its pixel tiles and adds them to the float32 result at the end.
namespace {

#ifndef WRW_DEPTH
#define WRW_DEPTH 2 // operand fragments requested ahead of the one being multiplied: 1: 603, 2: 676, 3: 654, 4: 635 TFLOP/s at
                    // 32 x 640 x 200 (one fragment ahead left every step waiting out most of an LDS round trip)
#endif

template <int Q> __device__ __forceinline__ void wrw_issue(tr_frag &f, const unsigned ga, const unsigned xa)
{
    constexpr int ks_ = Q / 10, j_ = Q % 10, rr_ = ks_ >> 1, hw_ = ks_ & 1;
    if constexpr (j_ == 0) LDS_TR_ISSUE(f, ga, 2 * ((rr_ * WT_W + 16 * hw_) * ROW));
    else LDS_TR_ISSUE(f, xa, 2 * (((rr_ + (j_ - 1) / 3) * WHALO_W + 16 * hw_ + (j_ - 1) % 3) * ROW));
}

// (A variant in which a wave owns both co halves and a group of 4 - 5 taps -- 0.72 instead of 1.11 fragment reads per MFMA --
// measured no faster, 621 - 648 TFLOP/s: the LDS read rate is not what this kernel waits for.)
template <int Q>
__device__ __forceinline__ void wrw_steps(tr_frag (&fr)[WRW_DEPTH + 1], bf16x8 &a, f32x16 (&acc)[9], const unsigned ga, const unsigned xa)
{
    constexpr int R = WRW_DEPTH + 1;
    if constexpr (Q < 80) {
        if constexpr (Q + WRW_DEPTH < 80) wrw_issue<Q + WRW_DEPTH>(fr[(Q + WRW_DEPTH) % R], ga, xa);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (Q % 10 == 0) a = tr_value(fr[Q % R]);
        else acc[Q % 10 - 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, tr_value(fr[Q % R]), acc[Q % 10 - 1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (Q + 1 < 80) { // fragment Q+1 must have landed; the younger ones (two reads each) may still be in flight
            constexpr int younger = (Q + WRW_DEPTH < 80 ? WRW_DEPTH : 79 - Q) - 1;
            if constexpr (younger <= 0) LDS_TR_WAIT_N(fr[(Q + 1) % R], 0);
            else if constexpr (younger == 1) LDS_TR_WAIT_N(fr[(Q + 1) % R], 2);
            else if constexpr (younger == 2) LDS_TR_WAIT_N(fr[(Q + 1) % R], 4);
            else LDS_TR_WAIT_N(fr[(Q + 1) % R], 6);
        }
        wrw_steps<Q + 1>(fr, a, acc, ga, xa);
    }
}

// XF (round 4): x is the RAW output x1 of the convolution before and the operand is a = dropout(relu(batch_norm(x1))), formed in
// registers between the global load and the LDS write of each piece (this kernel stages through registers): see XformArgs.
template <bool XF>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_wrw_kernel(const unsigned short *__restrict__ x,
                                                                 const unsigned short *__restrict__ dy,
                                                                 float *__restrict__ dw, int N, int H, int W, const Geo geo,
                                                                 float *__restrict__ part /* deterministic mode: [gridDim.x][64*9*64] */,
                                                                 const XformArgs xf)
{
    __shared__ __attribute__((aligned(16))) unsigned short xl[WHALO_H * WHALO_W * ROW];
    __shared__ __attribute__((aligned(16))) unsigned short gl[WT_H * WT_W * ROW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int mb = wv & 1, nb = wv >> 1;                 // this wave: co 32*mb.., ci 32*nb..
    const int i16 = lane & 15, cb = (lane >> 4) & 1, kh = lane >> 5;
    // per-lane source address inside a 16-pixel x 32-channel operand block (see the comment above)
    const unsigned a_lane = 2u * (unsigned)((8 * kh + (i16 >> 2)) * ROW + 32 * mb + 16 * cb + 4 * (i16 & 3));
    const unsigned b_lane = 2u * (unsigned)((8 * kh + (i16 >> 2)) * ROW + 32 * nb + 16 * cb + 4 * (i16 & 3));
    const unsigned gbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)gl;
    const unsigned xbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)xl;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; t++) acc[t] = f32x16{};
    const int tiles_w = (W + WT_W - 1) / WT_W, tiles_h = (H + WT_H - 1) / WT_H;
    constexpr int XP = (WHALO_H * WHALO_W * 8 + 255) / 256, GP = WT_H * WT_W * 8 / 256; // 16-byte pieces per thread
    uint4 px_[XP], pg_[GP];
    // Round 3: the fetch used to decode the tile with 64-bit divisions and rebuild a 64-bit address with a division by 34 for
    // every one of its 11 loads -- ~45 instructions per load, as many issue cycles per tile as the 72 MFMAs (probe builds at
    // 32 x 640 x 200: 0.445 ms, 0.252 without the fetch, 0.242 without the multiply, 0.114 with neither: purely additive).
    // Now a cursor steps (tw, th, n) by the grid size with carries, the tile's origin is ONE wave-uniform 64-bit pointer, and a
    // load is that pointer + a 32-bit offset from the thread's halo position (q / 34 by multiply-shift, exact for q < 236).
    struct Cursor { int tw, th, n; };
    const TileWalk walk = tile_walk(N, tiles_h, tiles_w, (int)gridDim.x, (int)blockIdx.x); // XCD-aware order (see tile_walk)
    const int stride_ = walk.G;
    auto cursor_of = [&](const TilePos &p) {
        Cursor c;
        c.tw = p.tw;
        tile_coords(walk, p, c.n, c.th);
        return c;
    };
    static_assert(WHALO_W == 34 && WHALO_H * WHALO_W + 31 < 236, "q / 34 == (q * 241) >> 13 holds for q < 236");
    auto fetch = [&](const Cursor &c) { // one tile's x (with halo, zeros outside the image) and dy into registers
        const int h0 = c.th * WT_H, w0 = c.tw * WT_W;
        const unsigned short *xo = x + geo_off(geo, c.n, h0 - 1, w0 - 1);   // halo pixel (0, 0); wave-uniform
        const unsigned short *go = dy + geo_off(geo, c.n, h0, w0);
        const int p0 = tid >> 3, piece8 = (tid & 7) * 8;
#pragma unroll
        for (int j = 0; j < XP; j++) {
            const int q = p0 + 32 * j;                   // halo pixel of this piece, row-major in the 6 x 34 halo
            const int hh = (q * 241) >> 13, ww = q - hh * WHALO_W;
            const bool ok = q < WHALO_H * WHALO_W && (unsigned)(h0 - 1 + hh) < (unsigned)H && (unsigned)(w0 - 1 + ww) < (unsigned)W;
            px_[j] = make_uint4(0u, 0u, 0u, 0u);
#ifndef WRW64_NO_FETCH // (probe builds: WRW64_NO_FETCH / WRW64_NO_LDSWRITE / WRW64_NO_MULT drop one phase each)
            if (ok) px_[j] = *(const uint4 *)(xo + (hh * geo.sh + ww * geo.sw + piece8));
#endif
        }
#pragma unroll
        for (int j = 0; j < GP; j++) {
            const int q = p0 + 32 * j, hh = q >> 5, ww = q & 31;
            pg_[j] = make_uint4(0u, 0u, 0u, 0u);
#ifndef WRW64_NO_FETCH
            if (h0 + hh < H && w0 + ww < W) pg_[j] = *(const uint4 *)(go + (hh * geo.sh + ww * geo.sw + piece8));
#endif
        }
    };
    const int n_local = walk.n_local;                // tiles of this workgroup's XCD; `tile` = position in that sequence
    int tile = (int)blockIdx.x / walk.nx;
    TilePos pcur = tile_pos(walk, tile);
    __shared__ __attribute__((aligned(16))) float xtab[XF ? 2 * 64 : 4]; // XF: scale[64], shift[64]
    if (XF) {
        if (tid < 64) {
            const float sc = xf.invstd[tid] * xf.gamma[tid];
            xtab[tid] = sc;
            xtab[64 + tid] = xf.beta[tid] - xf.mean[tid] * sc;
        }
    } // (the loop's first __syncthreads() publishes the table)
    if (tile < n_local) fetch(cursor_of(pcur));
    for (; tile < n_local; tile += stride_) {
        __syncthreads(); // the previous tile's LDS reads are done
#ifndef WRW64_NO_LDSWRITE
        if (XF) { // a = dropout(relu(x1 * scale + shift)) on the pieces inside the image (outside: the zero padding of the ACTIVATION)
            const Cursor c = cursor_of(pcur);
            const int h0 = c.th * WT_H, w0 = c.tw * WT_W;
            const long origin = geo_off(geo, c.n, h0 - 1, w0 - 1);
            const int p0 = tid >> 3, piece8 = (tid & 7) * 8;
            const float4 s0 = *(const float4 *)(xtab + piece8), s1 = *(const float4 *)(xtab + piece8 + 4);
            const float4 t0 = *(const float4 *)(xtab + 64 + piece8), t1 = *(const float4 *)(xtab + 64 + piece8 + 4);
            const float xsc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, xsh[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int j = 0; j < XP; j++) {
                const int q = p0 + 32 * j;
                const int hh = (q * 241) >> 13, ww = q - hh * WHALO_W;
                const bool ok = q < WHALO_H * WHALO_W && (unsigned)(h0 - 1 + hh) < (unsigned)H && (unsigned)(w0 - 1 + ww) < (unsigned)W;
                if (ok) {
                    const long e0 = origin + (long)hh * geo.sh + (long)ww * geo.sw + piece8;
                    const unsigned in[4] = {px_[j].x, px_[j].y, px_[j].z, px_[j].w};
                    unsigned out[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        float a = fmaxf(__uint_as_float(in[k] << 16) * xsc[2 * k] + xsh[2 * k], 0.f);
                        float b = fmaxf(__uint_as_float(in[k] & 0xffff0000u) * xsc[2 * k + 1] + xsh[2 * k + 1], 0.f);
                        if (xf.drop.thresh) {
                            const unsigned hsh = drop_hash((unsigned)(e0 >> 1) + k, xf.drop.seed);
                            a = (hsh & 0xFFFFu) >= xf.drop.thresh ? a * xf.drop.scale : 0.f;
                            b = (hsh >> 16) >= xf.drop.thresh ? b * xf.drop.scale : 0.f;
                        }
                        out[k] = pack_bf16(a, b);
                    }
                    px_[j] = make_uint4(out[0], out[1], out[2], out[3]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < XP; j++) {
            const int i = tid + j * 256;
            if (i < WHALO_H * WHALO_W * 8) *(uint4 *)(xl + (long)(i >> 3) * ROW + (i & 7) * 8) = px_[j];
        }
#pragma unroll
        for (int j = 0; j < GP; j++) {
            const int i = tid + j * 256;
            *(uint4 *)(gl + (long)(i >> 3) * ROW + (i & 7) * 8) = pg_[j];
        }
#endif
        __syncthreads();
        tile_advance(walk, pcur);
        if (tile + stride_ < n_local) fetch(cursor_of(pcur)); // in flight during the multiply below
        // 8 K-steps (4 rows x 2 halves of 16 consecutive pixels) x 9 taps, software-pipelined by hand like the forward kernel:
        // the fragment of step q+1 is requested before step q's MFMA issues.  Step q = ks * 10 + j: j = 0 is the dy
        // fragment of K-step ks, j = 1..9 the x fragment of tap j-1.
        const unsigned ga = gbase + a_lane, xa = xbase + b_lane;
        tr_frag fr[WRW_DEPTH + 1];
        bf16x8 a;
        wrw_issue<0>(fr[0], ga, xa);
        if constexpr (WRW_DEPTH >= 2) wrw_issue<1>(fr[1], ga, xa);
        if constexpr (WRW_DEPTH >= 3) wrw_issue<2>(fr[2], ga, xa);
        if constexpr (WRW_DEPTH >= 4) wrw_issue<3>(fr[3], ga, xa);
        if constexpr (WRW_DEPTH == 1) LDS_TR_WAIT_N(fr[0], 0);
        else if constexpr (WRW_DEPTH == 2) LDS_TR_WAIT_N(fr[0], 2);
        else if constexpr (WRW_DEPTH == 3) LDS_TR_WAIT_N(fr[0], 4);
        else LDS_TR_WAIT_N(fr[0], 6);
#ifndef WRW64_NO_MULT
        wrw_steps<0>(fr, a, acc, ga, xa);
#else
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    }
    // D[m = co][n = ci]: column = lane&31 = ci, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) = co within the block
#ifndef WRW64_NO_ATOMIC // (probe)
    if (part) {
        // deterministic mode: the workgroup's 64 x 9 x 64 block goes to its slab.  Written as the accumulators lie that is 144
        // scattered 4-byte stores per lane (the wide kernel's probe builds: a quarter of the launch); instead each tap's 64 x 64
        // plane is turned through LDS (the x tile's buffer is free) into its memory layout and written as 16-byte stores,
        // whole 256-byte rows (round 4)
        float *blk = (float *)xl; // [64 co][64 ci]
        static_assert(sizeof(xl) >= 64 * 64 * 4, "one tap's plane");
        float *out = part + (long)blockIdx.x * (64L * 9 * 64);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            __syncthreads();
#pragma unroll
            for (int reg = 0; reg < 16; reg++)
                blk[(32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)) * 64 + 32 * nb + (lane & 31)] = acc[tap][reg];
            __syncthreads();
            const int ft = geo.tap_t ? (tap % 3) * 3 + tap / 3 : tap; // (transposed geometry: tap (ky, kx) is the filter's (kx, ky))
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int co = 16 * r + (tid >> 4), seg = tid & 15;
                *(float4 *)(out + ((long)(co * 9 + ft)) * CH + seg * 4) = *(const float4 *)(blk + co * 64 + seg * 4);
            }
        }
        return;
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int co = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), ci = 32 * nb + (lane & 31);
            atomicAdd(dw + ((long)(co * 9 + (geo.tap_t ? (tap % 3) * 3 + tap / 3 : tap)) * CH + ci), acc[tap][reg]);
        }
#endif
}

} // namespace

#ifndef C64_WRW_MID
#define C64_WRW_MID 256 // persistent workgroups of the weight gradient at 4096 .. 16383 tiles, and (C64_WRW_BIG) beyond; with slabs (round 4) at
                        // 32 x 320 x 100: 256: 99 us, 384: 105, 512: 101 (the launch + its slab reduction); with atomics 384 was best
#endif
#ifndef C64_WRW_BIG
#define C64_WRW_BIG 512
#endif
// dw: float32 [64 co][3][3][64 ci], ADDED to (zero it first); x, dy: [N][H][W][64] bf16
extern "C" int salsa_nn_conv3x3_c64_wrw(const void *x, const void *dy, float *dw, int64_t N, int H, int W, void *hip_stream)
{
    if (!x || !dy || !dw || N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH) return -1;
    const C64Plan pl = c64_plan(N, H, W, WT_H, WT_W);
    const long tiles = pl.tiles;
    // persistent workgroups, two per CU; fewer when there are few tiles (every workgroup ends with 36 864 float atomics)
    // (mid sizes, 32 x 320 x 100: 256 workgroups 0.158 ms, 384: 0.141, 512: 0.149)
    const unsigned nb = (unsigned)(tiles >= 16384 ? C64_WRW_BIG : tiles >= 4096 ? C64_WRW_MID : tiles >= 128 ? 128 : tiles);
    int rc = 0;
    float *part = salsa_nn_det_begin((int)nb, 64L * 9 * 64, (hipStream_t)hip_stream, &rc);
    if (rc) return rc;
    hipLaunchKernelGGL(conv3x3_c64_wrw_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned short *)x,
                       (const unsigned short *)dy, dw, (int)N, pl.Hk, pl.Wk, pl.geo, part, XformArgs{});
    if (part) return salsa_nn_det_finish(part, (int)nb, 64L * 9 * 64, dw, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// The same with x = the RAW output x1 of the convolution before and the operand a = dropout(relu(batch_norm(x1))) formed on the
// fly (mean / invstd: the BatchNorm's batch statistics, salsa_nn_bn_train_finalize; drop_p / drop_seed as salsa_nn_bn_train_fwd).
extern "C" int salsa_nn_conv3x3_c64_wrw_xform(const void *x1, const void *dy, float *dw, const float *mean, const float *invstd,
                                              const float *gamma, const float *beta, float drop_p, uint32_t drop_seed, int64_t N, int H,
                                              int W, void *hip_stream)
{
    if (!x1 || !dy || !dw || !mean || !invstd || !gamma || !beta || drop_p < 0.f || drop_p >= 1.f || N <= 0 || H <= 0 || W <= 0 ||
        N * H * W >= INT32_MAX / CH)
        return -1;
    const C64Plan pl = c64_plan(N, H, W, WT_H, WT_W);
    const long tiles = pl.tiles;
    const unsigned nb = (unsigned)(tiles >= 16384 ? C64_WRW_BIG : tiles >= 4096 ? C64_WRW_MID : tiles >= 128 ? 128 : tiles);
    int rc = 0;
    float *part = salsa_nn_det_begin((int)nb, 64L * 9 * 64, (hipStream_t)hip_stream, &rc);
    if (rc) return rc;
    const XformArgs xf = {mean, invstd, gamma, beta, drop_args(drop_p, drop_seed)};
    hipLaunchKernelGGL(conv3x3_c64_wrw_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned short *)x1,
                       (const unsigned short *)dy, dw, (int)N, pl.Hk, pl.Wk, pl.geo, part, xf);
    if (part) return salsa_nn_det_finish(part, (int)nb, 64L * 9 * 64, dw, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
