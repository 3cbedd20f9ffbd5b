// conv_stem_wrw.hip -- weight gradient of the CRNN's first convolution (conv_stem.hip), Cin <= 14 -> 64, on the gfx950 matrix
// cores; alone, with the BatchNorm (+ ReLU) backward behind it applied on the fly, or with that backward folded in whole.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nn_det.h"
#include "conv_internal.h"

// ------------------------------------------------------------------------------------------ weight gradient, first layer
// dW[co][ci][tap] = sum_p dy[p][co] * x[ci][p + tap] for the (Cin <= 7) -> 64 first layer: the same pixel-reduction GEMM as
// above with N = Cin*9 <= 63 columns (one 64-column block, column c = ci*9 + tap; column 63 multiplies a zero plane).  The A
// operand (dy^T) comes from the pixel-major dy tile through transposing LDS reads exactly as in the 64 -> 64 kernel.  The B
// operand needs, per lane, 8 consecutive pixels of ONE (ci, tap) -- and x is float32 PLANAR (the extractor's layout: no bf16
// channels-last copy of the input is made for this kernel), so consecutive pixels ARE consecutive floats: the tile's halo is
// converted to bf16 once and stored in LDS as three column-shifted copies per (ci, halo row), which makes every fragment one
// aligned 16-byte read.  33.5 GFLOP against 0.64 GB of input: HBM-bound; a wave owns one 32 x 32 block of dW.
namespace {

// CB = column blocks of 64: 1 for Cin <= 7 (the SALSA path), 2 for 8 <= Cin <= 14 (the baseline GCC features' 10 channels: 90 of
// 128 columns).  With CB = 2 a wave owns two 32 x 32 blocks of dW (columns 32 nb + 64 cb) that share every A fragment.
constexpr int SW_XROW = 40;                               // bf16 per (ci, halo row, shift) row: 32 + pad (80-byte pitch)
template <int CB> constexpr int SW_XS = 8 * CB * WHALO_H * 3 * SW_XROW; // 8 CB channel planes (those >= Cin stay zero)
template <int CB> constexpr int SW_XPF = (7 * CB * WHALO_H * WHALO_W + 255) / 256; // float32 halo elements per thread

template <int CB, int KS>
__device__ __forceinline__ void stem_wrw_steps(f32x16 (&acc)[CB], const unsigned ga, const unsigned (&xa)[CB])
{
    if constexpr (KS < 8) {
        constexpr int rr = KS >> 1, hw = KS & 1;
        tr_frag fa;
        bf16x8 b[CB];
        LDS_TR_ISSUE(fa, ga, 2 * ((rr * WT_W + 16 * hw) * ROW));
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b[cb]) : "v"(xa[cb]), "n"(2 * (rr * 3 * SW_XROW + 16 * hw)));
        if constexpr (CB == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa.lo), "+v"(fa.hi), "+v"(b[0]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa.lo), "+v"(fa.hi), "+v"(b[0]), "+v"(b[1]));
#pragma unroll
        for (int cb = 0; cb < CB; cb++) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_value(fa), b[cb], acc[cb], 0, 0, 0);
        stem_wrw_steps<CB, KS + 1>(acc, ga, xa);
    }
}

// MODE 2 (see the kernel): the same input fragment against the masked-gradient tile and the normalised-activation tile; its eight
// values also go into this lane's share of S0 (v_dot2_f32_bf16 with a pair of ones: one register, where a third product against a
// fragment of ones would cost sixteen)
// S0 must leave out the OUTPUT pixels of a tile that hang over the image's right / bottom edge by itself (G and Xh see g = xh = 0
// there, but those pixels' input patches next to the edge are real): om[hw][q] = the pair of ones for pixel pair q of the lane's eight
// pixels in column half hw (zero where the pixel is outside), rows outside (rr >= h_left) are dropped per row.
template <int CB, int KS>
__device__ __forceinline__ void stem_wrw_steps2(f32x16 (&acc_g)[CB], f32x16 (&acc_x)[CB], float (&s0)[CB], float (&t)[CB], const unsigned ga,
                                                const unsigned ga2, const unsigned (&xa)[CB], const unsigned (&om)[2][4], const int h_left)
{
    if constexpr (KS < 8) {
        constexpr int rr = KS >> 1, hw = KS & 1;
        tr_frag fa, fx;
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        u32x4_t b[CB];
        LDS_TR_ISSUE(fa, ga, 2 * ((rr * WT_W + 16 * hw) * ROW));
        LDS_TR_ISSUE(fx, ga2, 2 * ((rr * WT_W + 16 * hw) * ROW));
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(b[cb]) : "v"(xa[cb]), "n"(2 * (rr * 3 * SW_XROW + 16 * hw)));
        if constexpr (CB == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa.lo), "+v"(fa.hi), "+v"(fx.lo), "+v"(fx.hi), "+v"(b[0]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(fa.lo), "+v"(fa.hi), "+v"(fx.lo), "+v"(fx.hi), "+v"(b[0]), "+v"(b[1]));
#pragma unroll
        for (int cb = 0; cb < CB; cb++) {
            const bf16x8 bv = __builtin_bit_cast(bf16x8, b[cb]);
            acc_g[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_value(fa), bv, acc_g[cb], 0, 0, 0);
            acc_x[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_value(fx), bv, acc_x[cb], 0, 0, 0);
        }
        // (one asm statement with its own trailing wait states: a dot product's result needs them before an ordinary vector
        // instruction may read it, and the compiler's hazard recognizer cannot see into asm statements -- four separate ones let the
        // add below read t too early; the builtin form was worse: the compiler then read the fragment's registers after re-using them)
#pragma unroll
        for (int cb = 0; cb < CB; cb++) {
            if (hw == 0) t[cb] = 0.f;
            asm volatile("v_dot2_f32_bf16 %0, %1, %5, %0\n\tv_dot2_f32_bf16 %0, %2, %6, %0\n\tv_dot2_f32_bf16 %0, %3, %7, %0\n\t"
                         "v_dot2_f32_bf16 %0, %4, %8, %0\n\ts_nop 4"
                         : "+v"(t[cb])
                         : "v"(b[cb].x), "v"(b[cb].y), "v"(b[cb].z), "v"(b[cb].w), "v"(om[hw][0]), "v"(om[hw][1]), "v"(om[hw][2]), "v"(om[hw][3]));
            if (hw == 1) s0[cb] += rr < h_left ? t[cb] : 0.f;
        }
        stem_wrw_steps2<CB, KS + 1>(acc_g, acc_x, s0, t, ga, ga2, xa, om, h_left);
    }
}
struct StemBnf { const float *mean, *invstd, *gamma, *beta; }; // MODE 2: the forward's statistics and the affine parameters [64]
// MODE 2: a workgroup's partial sums: G[64][64 CB] (last column = dbeta), Xh[64][64 CB], S0[2][64 CB], dgamma[64]
template <int CB> constexpr int SW_SLAB = 2 * 64 * 64 * CB + 2 * 64 * CB + 64;

// BN: dy is not the gradient of the convolution's output but of the BatchNorm (+ ReLU) output behind it, and x1 that
// BatchNorm's input (= this convolution's output): the tile's dx = a (g masked - b - (x1 - mean) k) -- the BatchNorm backward's
// apply pass, coefficients from salsa_nn_bn_bwd(dx = NULL) -- is formed while the tile goes into LDS, rounded to bf16 exactly
// as the separate pass would have stored it.  This layer's weight gradient is dx's ONLY reader (the network input needs no
// gradient), so the 524-MB dx is never written or read: 4 tensor passes become 2.
// MODE 2 (round 5): the BatchNorm backward's REDUCTION pass folded in as well.  dx = a (g - b - xh k') is linear in the two totals
// b = mean(g), k' = mean(g xh) that are only known after a pass over (g, x1) -- the pass this kernel makes anyway.  So it multiplies
// the input patches with the masked gradient g AND with the normalised activation xh = (x1 - mean) invstd,
//     G[co][c] = sum_p g[p][co] patch[p][c],   Xh[co][c] = sum_p xh[p][co] patch[p][c],   S0[c] = sum_p patch[p][c]  (v_dot2 on the side),
// gets dbeta = sum g as G's column 63 (the spare eighth input plane holds ones) and adds up dgamma = sum g xh on the way; a small
// launch afterwards combines the workgroups' partial sums:
//     dW[co][c] = a[co] (G[co][c] - b[co] S0[c] - k'[co] Xh[co][c]),   a = gamma invstd.
// The salsa_nn_bn_bwd(dx = NULL) launch (a second read of the 524-MB g and x1, ~145 us) disappears; the operands are g (exact in
// bf16) and bf16(xh) where MODE 1 rounds dx to bf16: the same order of rounding error.
// CB = 2, MODE 2 holds four accumulator tiles per wave and the doubled halo loads: bound to one wave per SIMD (512 registers).
template <int MODE, int CB = 1>
#ifndef STEM_WRW_WPS
#define STEM_WRW_WPS 1
#endif
__global__ __launch_bounds__(256, MODE == 2 && CB == 1 ? 2 : STEM_WRW_WPS) void conv3x3_stem_wrw_kernel(const float *__restrict__ x, long xbs, long xcs,
                                                               const unsigned short *__restrict__ dy, float *__restrict__ dw,
                                                               int N, int Cin, int H, int W,
                                                               const unsigned short *__restrict__ x1, const float *__restrict__ coef,
                                                               int relu, float *__restrict__ part /* deterministic mode: [gridDim.x][64*Cin*9]; MODE 2: [gridDim.x][SW_SLAB] */,
                                                               const StemBnf bnf)
{
    constexpr bool BN = MODE != 0;
    // (8 spare elements in front: the halo conversion stores every element into all three shifted copies UNCONDITIONALLY -- columns
    // -2, -1, 32, 33 land in the 8 padding columns of this row or of the one before, which nothing reads; behind `0 <= col < 32`
    // each of the 18 stores was an EXEC-mask region of its own)
    __shared__ __attribute__((aligned(16))) unsigned short xs_raw[SW_XS<CB> + 8];
    unsigned short *const xs = xs_raw + 8;
    __shared__ __attribute__((aligned(16))) unsigned short gl[WT_H * WT_W * ROW];
    __shared__ __attribute__((aligned(16))) unsigned short gl2[MODE == 2 ? WT_H * WT_W * ROW : 8]; // MODE 2: the xh tile

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int mb = wv & 1, nb = wv >> 1; // this wave: co 32*mb.., columns 32*nb..
    const int i16 = lane & 15, cb = (lane >> 4) & 1, kh = lane >> 5;
    const unsigned a_lane = 2u * (unsigned)((8 * kh + (i16 >> 2)) * ROW + 32 * mb + 16 * cb + 4 * (i16 & 3));
    constexpr int NCOL = 64 * CB, ONES = (NCOL - 1) / 9; // columns; MODE 2: the spare plane of ones (7 / 14)
    int c[CB];
    unsigned xa[CB];
    const unsigned ga = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)gl + a_lane;
#pragma unroll
    for (int cb = 0; cb < CB; cb++) { // last column: ci = ONES, a zero plane (Cin <= 7 / 14)
        c[cb] = 32 * nb + 64 * cb + (lane & 31);
        const int ci = c[cb] / 9, tap = c[cb] - 9 * ci;
        const unsigned b_lane = 2u * (unsigned)(((ci * WHALO_H + tap / 3) * 3 + tap % 3) * SW_XROW + 8 * kh);
        xa[cb] = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)xs + b_lane;
    }
    const unsigned ga2 = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)gl2 + a_lane;
    for (int i = tid; i < SW_XS<CB> / 8; i += 256) ((uint4 *)xs)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (MODE == 2) { // the spare input plane ONES holds ones: G[co][NCOL - 1] = sum_p g[p][co] = dbeta
        __syncthreads();
        for (int i = tid; i < WHALO_H * 3 * SW_XROW; i += 256) xs[ONES * WHALO_H * 3 * SW_XROW + i] = 0x3F80;
    }
    f32x16 acc[CB], acc_x[CB];
#pragma unroll
    for (int cb = 0; cb < CB; cb++) { acc[cb] = f32x16{}; acc_x[cb] = f32x16{}; }
    float s0[CB]; // MODE 2: this lane's share of S0[c] (its half of the k-steps' pixels)
#pragma unroll
    for (int cb = 0; cb < CB; cb++) s0[cb] = 0.f;
    float s_dg[8];   // MODE 2: this thread's share of dgamma (its pieces always cover the same 8 channels)
#pragma unroll
    for (int e = 0; e < 8; e++) s_dg[e] = 0.f;
    const int tiles_w = (W + WT_W - 1) / WT_W, tiles_h = (H + WT_H - 1) / WT_H;
    const long n_tiles = (long)N * tiles_h * tiles_w;
    constexpr int GP = WT_H * WT_W * 8 / 256;
    const int n_x = Cin * WHALO_H * WHALO_W;
    // Round 5: TWO register sets of tile loads in flight (the tile after next is fetched while this one is converted and
    // multiplied) and raw barriers.  Before: one set, fetched after the second __syncthreads() of a tile and needed right after the
    // first one of the next -- a fence + barrier = s_waitcnt vmcnt(0), so every tile exposed a whole memory latency minus eight
    // MFMAs, at two resident workgroups per CU (185 registers).  The second set costs 38 registers the kernel had spare at that
    // occupancy.  Every load is unconditional (a clamped in-bounds address; validity bits applied at conversion), so that nothing
    // but loads sits between the loads of a set.
    struct TileRegs {
        float px[SW_XPF<CB>];
        uint4 pg[GP], pq[BN ? GP : 1];
        unsigned okx, okg; // validity bits of the halo elements / the tile pieces
        int th, tw;
    };
    // Tile coordinates by a cursor that steps by the grid size with carries (decoding every tile index with 64-bit divisions --
    // tile % tiles_w, (tile / tiles_w) % tiles_h, tile / (tiles_w tiles_h) -- was ~230 scalar instructions per tile on one dependent
    // chain).  Past the end the cursor stays on the last tile (fetched, never used).
    struct Cursor { int tw, th, n; long t; };
    const long G = gridDim.x, t_last = n_tiles - 1;
    const int dgw = (int)(G % tiles_w), dgh = (int)((G / tiles_w) % tiles_h), dgn = (int)(G / ((long)tiles_w * tiles_h));
    auto cursor_at = [&](long t) {
        Cursor c;
        c.t = t; c.tw = (int)(t % tiles_w); c.th = (int)((t / tiles_w) % tiles_h); c.n = (int)(t / ((long)tiles_w * tiles_h));
        return c;
    };
    const Cursor c_last = cursor_at(t_last);
    auto advance = [&](Cursor &c) { // + G, clamped to the last tile
        c.t += G;
        c.tw += dgw;
        if (c.tw >= tiles_w) { c.tw -= tiles_w; c.th += 1; }
        c.th += dgh;
        if (c.th >= tiles_h) { c.th -= tiles_h; c.n += 1; }
        c.n += dgn;
        if (c.t >= t_last) c = c_last;
    };
    auto fetch = [&](const Cursor &tile, TileRegs &r) {
        const int tw = tile.tw, th = tile.th;
        const long n = tile.n;
        const int h0 = th * WT_H, w0 = tw * WT_W;
        r.th = th; r.tw = tw; r.okx = 0u; r.okg = 0u;
        // one wave-uniform 64-bit base per tensor and image + a 32-bit offset per load, validity by unsigned compares joined with `&`:
        // written with `&&` and 64-bit element offsets every load was three nested EXEC-mask regions around three 64-bit multiply-adds
        const float *xb = x + n * xbs;
        const long pix0 = n * H * W * CH;
        const unsigned short *gb = dy + pix0, *qb = BN ? x1 + pix0 : nullptr;
        const int xcs32 = (int)xcs;
#pragma unroll
        for (int j = 0; j < SW_XPF<CB>; j++) {
            const int i = tid + j * 256, cc = i / (WHALO_H * WHALO_W), rr = i - cc * (WHALO_H * WHALO_W);
            const int hh = rr / WHALO_W, ww = rr - hh * WHALO_W;
            const int h = h0 + hh - 1, wc = w0 + ww - 1;
            const bool ok = (i < n_x) & ((unsigned)h < (unsigned)H) & ((unsigned)wc < (unsigned)W);
            r.okx |= (ok ? 1u : 0u) << j;
            r.px[j] = xb[ok ? (unsigned)(cc * xcs32 + h * W + wc) : 0u];
        }
#pragma unroll
        for (int j = 0; j < GP; j++) {
            const int i = tid + j * 256, piece = i & 7, p = i >> 3;
            const int hh = p / WT_W, ww = p - hh * WT_W;
            const int h = h0 + hh, wc = w0 + ww;
            const bool ok = (h < H) & (wc < W);
            r.okg |= (ok ? 1u : 0u) << j;
            const unsigned off = (ok ? (unsigned)((h * W + wc) * CH) : 0u) + (unsigned)(piece * 8);
            r.pg[j] = *(const uint4 *)(gb + off);
            if (BN) r.pq[j] = *(const uint4 *)(qb + off);
        }
    };
    // one bf16 pair of the tile: BatchNorm-backward apply on (g, x1) -> dx, rounded to bf16 (a pixel outside the image has
    // g = x1 = 0 and would give -a (b - mean k): the caller zeroes those pieces instead).  A thread's pieces always cover the
    // same 8 channels (piece index = tid & 7), so their 56 coefficients live in registers (a table in LDS cost seven LDS reads
    // per element: 0.43 ms for this kernel); the arithmetic is bn_bwd_apply_kernel's, operation for operation.
    float c_a[8], c_b[8], c_mu[8], c_k[8], c_is[8], c_be[8], c_ga[8];
    if (MODE == 1) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int ch = (tid & 7) * 8 + e;
            c_a[e] = coef[ch]; c_b[e] = coef[CH + ch]; c_mu[e] = coef[2 * CH + ch]; c_k[e] = coef[3 * CH + ch];
            c_is[e] = coef[4 * CH + ch]; c_be[e] = coef[5 * CH + ch]; c_ga[e] = coef[6 * CH + ch];
        }
    }
    if (MODE == 2) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int ch = (tid & 7) * 8 + e;
            c_mu[e] = bnf.mean[ch]; c_is[e] = bnf.invstd[ch]; c_ga[e] = bnf.gamma[ch]; c_be[e] = bnf.beta[ch];
            c_a[e] = c_b[e] = c_k[e] = 0.f;
        }
    }
    // MODE 2: one bf16 pair of the tile -> the masked gradient pair (returned) and the normalised-activation pair (xh2), both as the
    // matrix operands; dgamma from the unrounded float32 values, as bn_bwd_reduce_kernel forms it
    auto bnf_pair = [&](const unsigned g2, const unsigned q2, const int e0, const bool inside, unsigned &xh2, float &dg0, float &dg1) -> unsigned {
        const float g0 = __uint_as_float(g2 << 16), g1 = __uint_as_float(g2 & 0xffff0000u);
        const float x0 = __uint_as_float(q2 << 16), x1v = __uint_as_float(q2 & 0xffff0000u);
        const float xh0 = (x0 - c_mu[e0]) * c_is[e0], xh1 = (x1v - c_mu[e0 + 1]) * c_is[e0 + 1];
        const bool live0 = inside & !(relu && !(xh0 * c_ga[e0] + c_be[e0] > 0.f));
        const bool live1 = inside & !(relu && !(xh1 * c_ga[e0 + 1] + c_be[e0 + 1] > 0.f));
        const float gk0 = live0 ? g0 : 0.f, gk1 = live1 ? g1 : 0.f;
        asm("v_fmac_f32 %0, %1, %2" : "+v"(dg0) : "v"(gk0), "v"(xh0)); // (written out: left to the compiler the eight accumulators
        asm("v_fmac_f32 %0, %1, %2" : "+v"(dg1) : "v"(gk1), "v"(xh1)); //  cost the kernel ~100 registers -- 353 against 245)
        xh2 = pack_bf16(inside ? xh0 : 0.f, inside ? xh1 : 0.f);
        return pack_bf16(gk0, gk1); // (exact: g is a bf16 value or zero)
    };
    auto bn_pair = [&](const unsigned g2, const unsigned q2, const int e0) -> unsigned {
        float r[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const float g = __uint_as_float(e ? (g2 & 0xffff0000u) : (g2 << 16)), xv = __uint_as_float(e ? (q2 & 0xffff0000u) : (q2 << 16));
            const int ch = e0 + e;
            const float xc = xv - c_mu[ch];
            const bool zero = relu && !((xc * c_is[ch]) * c_ga[ch] + c_be[ch] > 0.f);
            r[e] = c_a[ch] * ((zero ? 0.f : g) - c_b[ch] - xc * c_k[ch]);
        }
        return pack_bf16(r[0], r[1]);
    };
    auto raw_barrier = [&]() { // LDS order only: the loads in flight stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // registers -> LDS: the halo as three column-shifted bf16 copies per (ci, row); the (g [, x1]) tile as dx rows
    auto convert = [&](const TileRegs &r) {
#pragma unroll
        for (int j = 0; j < SW_XPF<CB>; j++) {
            const int i = tid + j * 256, cc = i / (WHALO_H * WHALO_W), rr = i - cc * (WHALO_H * WHALO_W);
            const int hh = rr / WHALO_W, ww = rr - hh * WHALO_W;
            if (i < n_x) {
                const unsigned short bits = (unsigned short)(pack_bf16(((r.okx >> j) & 1u) ? r.px[j] : 0.f, 0.f) & 0xffffu); // round to nearest even
#pragma unroll
                for (int kx = 0; kx < 3; kx++) { // copy kx holds halo columns kx .. kx + 31 at positions 0 .. 31
                    xs[((cc * WHALO_H + hh) * 3 + kx) * SW_XROW + ww - kx] = bits;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < GP; j++) {
            const int i = tid + j * 256;
            const bool inside = (r.okg >> j) & 1u;
            uint4 v = r.pg[j];
            if (MODE == 1) {
                v.x = bn_pair(r.pg[j].x, r.pq[j].x, 0);
                v.y = bn_pair(r.pg[j].y, r.pq[j].y, 2);
                v.z = bn_pair(r.pg[j].z, r.pq[j].z, 4);
                v.w = bn_pair(r.pg[j].w, r.pq[j].w, 6);
            }
            if (MODE == 2) {
                uint4 u;
                v.x = bnf_pair(r.pg[j].x, r.pq[j].x, 0, inside, u.x, s_dg[0], s_dg[1]);
                v.y = bnf_pair(r.pg[j].y, r.pq[j].y, 2, inside, u.y, s_dg[2], s_dg[3]);
                v.z = bnf_pair(r.pg[j].z, r.pq[j].z, 4, inside, u.z, s_dg[4], s_dg[5]);
                v.w = bnf_pair(r.pg[j].w, r.pq[j].w, 6, inside, u.w, s_dg[6], s_dg[7]);
                *(uint4 *)(gl2 + (long)(i >> 3) * ROW + (i & 7) * 8) = u;
            } else if (!inside) v = make_uint4(0u, 0u, 0u, 0u);
            *(uint4 *)(gl + (long)(i >> 3) * ROW + (i & 7) * 8) = v;
        }
    };
    auto multiply = [&](const int th, const int tw) __attribute__((always_inline)) {
        if constexpr (MODE == 2) {
            const int h_left = H - th * WT_H, w_left = W - tw * WT_W;
            unsigned om[2][4];
#pragma unroll
            for (int hw = 0; hw < 2; hw++) {
                const int nv = w_left - (16 * hw + 8 * kh); // valid pixels among this lane's eight (<= 0: none, >= 8: all)
#pragma unroll
                for (int q = 0; q < 4; q++) om[hw][q] = (2 * q < nv ? 0x3F80u : 0u) | (2 * q + 1 < nv ? 0x3F800000u : 0u);
            }
            float t[CB];
#pragma unroll
            for (int cb = 0; cb < CB; cb++) t[cb] = 0.f;
            stem_wrw_steps2<CB, 0>(acc, acc_x, s0, t, ga, ga2, xa, om, h_left);
        } else stem_wrw_steps<CB, 0>(acc, ga, xa);
    };
    TileRegs ra, rb;
    long tile = blockIdx.x; // (< n_tiles: the launch has at most one workgroup per tile)
    // Every fetch is issued unconditionally (past the end: the last tile again, never converted): with a fetch or a tile behind a
    // branch the compiler's wait insertion merges the paths and drains BOTH sets (vmcnt 13 .. 0) where the older set alone
    // is needed (vmcnt 27 .. 14)
    Cursor nf = cursor_at(tile); // the next tile to request
    fetch(nf, ra);
    advance(nf);
    fetch(nf, rb);
    advance(nf);
    __syncthreads(); // the zero fill of xs (and nothing else: the loads above land in registers)
    for (; tile + G < n_tiles; tile += 2 * G) {
        raw_barrier(); // the previous tile's LDS reads are done
        convert(ra);
        raw_barrier();
        const int tha = ra.th, twa = ra.tw;
        fetch(nf, ra); // (tile + 2 G) in flight during this tile's multiply and the whole next tile
        advance(nf);
        multiply(tha, twa);
        raw_barrier();
        convert(rb);
        raw_barrier();
        const int thb = rb.th, twb = rb.tw;
        fetch(nf, rb); // (tile + 3 G)
        advance(nf);
        multiply(thb, twb);
    }
    if (tile < n_tiles) {
        raw_barrier();
        convert(ra);
        raw_barrier();
        multiply(ra.th, ra.tw);
    }
    if (MODE == 2) { // this workgroup's slab: G (column 63: dbeta), Xh, S0 (the two lane halves), dgamma
        float *slab = part + (long)blockIdx.x * SW_SLAB<CB>;
#pragma unroll
        for (int cb = 0; cb < CB; cb++) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int co = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                slab[co * NCOL + c[cb]] = acc[cb][reg];
                slab[64 * NCOL + co * NCOL + c[cb]] = acc_x[cb][reg];
            }
            if (mb == 0) slab[2 * 64 * NCOL + NCOL * kh + c[cb]] = s0[cb];
        }
        // dgamma: the 32 threads that share a channel group (tid & 7) through LDS, in a fixed order
        raw_barrier(); // (the last multiply's reads of gl are done)
        float *red = (float *)gl; // [8 values][256 threads]
#pragma unroll
        for (int e = 0; e < 8; e++) red[e * 256 + tid] = s_dg[e];
        __syncthreads();
        if (tid < 64) { // channel (tid & 7) * 8 + (tid >> 3)
            const int grp = tid & 7, v = tid >> 3;
            float t = 0.f;
            for (int q = 0; q < 32; q++) t += red[v * 256 + grp + 8 * q];
            slab[2 * 64 * NCOL + 2 * NCOL + grp * 8 + v] = t;
        }
        return;
    }
    // D[m = co][n = column]: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if constexpr (CB == 1) {
        if (c[0] < Cin * 9 && (long)blockIdx.x < n_tiles) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int co = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                salsa_nn_accumulate(dw, part, 64L * Cin * 9, (int)blockIdx.x, (long)co * (Cin * 9) + c[0], acc[0][reg]);
            }
        }
        return;
    }
#pragma unroll
    for (int cb = 0; cb < CB; cb++)
        if (c[cb] < Cin * 9 && (long)blockIdx.x < n_tiles) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int co = 32 * mb + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                salsa_nn_accumulate(dw, part, 64L * Cin * 9, (int)blockIdx.x, (long)co * (Cin * 9) + c[cb], acc[cb][reg]);
            }
        }
}

} // namespace

// dw: float32 [64 co][Cin][3][3] contiguous, ADDED to (zero it first); x float32 planar [N][Cin <= 14][H][W] (strides in elements,
// rows contiguous), dy bf16 channels-last [N][H][W][64]
extern "C" int salsa_nn_conv3x3_stem_wrw(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *dy, float *dw,
                                         int64_t N, int Cin, int H, int W, void *hip_stream)
{
    if (!x || !dy || !dw || N <= 0 || Cin <= 0 || Cin > 14 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH ||
        x_channel_stride < (int64_t)H * W || x_batch_stride < x_channel_stride * Cin ||
        x_channel_stride * Cin >= INT32_MAX /* 32-bit element offsets inside an image */)
        return -1;
    const long tiles = (long)N * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W);
    const unsigned nb = (unsigned)(tiles >= 1280 ? 1280 : tiles); // persistent, five per CU (30 KB of LDS each)
    int rc = 0;
    float *part = salsa_nn_det_begin((int)nb, 64L * Cin * 9, (hipStream_t)hip_stream, &rc);
    if (rc) return rc;
    hipLaunchKernelGGL((Cin <= 7 ? conv3x3_stem_wrw_kernel<0> : conv3x3_stem_wrw_kernel<0, 2>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, x, (long)x_batch_stride,
                       (long)x_channel_stride, (const unsigned short *)dy, dw, (int)N, Cin, H, W, (const unsigned short *)nullptr,
                       (const float *)nullptr, 0, part, StemBnf{});
    if (part) return salsa_nn_det_finish(part, (int)nb, 64L * Cin * 9, dw, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

#ifndef STEM_WRW_BN_GRID
#define STEM_WRW_BN_GRID 512
#endif
namespace {
// MODE 2's second launch: workgroup co adds the slabs' partial sums of its output channel in float64 -- thread (column k = tid & 63,
// slab lane tid >> 6) takes every 16th slab in ascending order, lane 0 then adds the 16 lanes' sums in lane order: a fixed order,
// bit-reproducible -- and combines them: dW[co][k] += a (G - b S0[k] - k' Xh), dbeta = sum g, dgamma = sum g xh.
// CB = 2: 128 columns, thread (k = tid & 127, slab lane tid >> 7), eight slab lanes.
template <int CB = 1>
__global__ __launch_bounds__(1024) void stem_wrw_bnf_finalize_kernel(const float *__restrict__ part, int nslab, double M, int ncol /* Cin * 9 */,
                                                                     const StemBnf bnf, float *__restrict__ dw, float *__restrict__ dgamma,
                                                                     float *__restrict__ dbeta)
{
    constexpr int NCOL = 64 * CB, NSL = 1024 / NCOL;
    __shared__ double red[5][1024];
    const int co = blockIdx.x, k = threadIdx.x & (NCOL - 1), sl = threadIdx.x / NCOL;
    double sg = 0.0, sx = 0.0, s0 = 0.0, sb = 0.0, sd = 0.0;
    for (int b0 = sl; b0 < nslab; b0 += NSL * 4) { // four slabs' loads in flight per thread; the additions keep their order
        float v[4][5];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int b = b0 + NSL * u;
            const float *q = part + (long)(b < nslab ? b : b0) * SW_SLAB<CB>;
            v[u][0] = q[co * NCOL + k];
            v[u][1] = q[64 * NCOL + co * NCOL + k];
            v[u][2] = q[2 * 64 * NCOL + k] + q[2 * 64 * NCOL + NCOL + k]; // S0: the two lane halves
            v[u][3] = q[co * NCOL + NCOL - 1];                              // dbeta: G's column of ones
            v[u][4] = q[2 * 64 * NCOL + 2 * NCOL + co];
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (b0 + NSL * u < nslab) {
                sg += (double)v[u][0]; sx += (double)v[u][1]; s0 += (double)v[u][2]; sb += (double)v[u][3]; sd += (double)v[u][4];
            }
    }
    red[0][threadIdx.x] = sg; red[1][threadIdx.x] = sx; red[2][threadIdx.x] = s0; red[3][threadIdx.x] = sb; red[4][threadIdx.x] = sd;
    __syncthreads();
    if (sl != 0) return;
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < NSL; q++)
#pragma unroll
        for (int a = 0; a < 5; a++) t[a] += red[a][q * NCOL + k];
    const double a = (double)bnf.gamma[co] * (double)bnf.invstd[co], bb = t[3] / M, kk = t[4] / M;
    if (k < ncol) dw[(long)co * ncol + k] += (float)(a * (t[0] - bb * t[2] - kk * t[1]));
    if (k == 0) {
        dbeta[co] = (float)t[3];
        dgamma[co] = (float)t[4];
    }
}
} // namespace

/* workspace of salsa_nn_conv3x3_stem_wrw_bnf: one slab of partial sums per workgroup */
extern "C" size_t salsa_nn_conv3x3_stem_wrw_bnf_ws_bytes(int64_t N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const long tiles = (long)N * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W);
    return sizeof(float) * SW_SLAB<1> * (size_t)(tiles >= STEM_WRW_BN_GRID ? STEM_WRW_BN_GRID : tiles);
}

// 8 <= Cin <= 14 (conv3x3_stem_wrw_kernel<2, 2>): one workgroup per CU is resident, so the grid is one round of 256
constexpr long STEM16_WRW_BN_GRID = 256;
/* the same for 8 <= Cin <= 14: larger slabs, a grid of its own */
extern "C" size_t salsa_nn_conv3x3_stem16_wrw_bnf_ws_bytes(int64_t N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const long tiles = (long)N * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W);
    return sizeof(float) * SW_SLAB<2> * (size_t)(tiles >= STEM16_WRW_BN_GRID ? STEM16_WRW_BN_GRID : tiles);
}

/* The first layer's weight gradient with the WHOLE BatchNorm (+ ReLU) backward behind it folded in (conv3x3_stem_wrw_kernel<2>): g =
 * gradient of the BatchNorm's output, x1 = its input, both bf16 channels-last; mean / invstd = the forward's saved statistics.  Leaves
 * dw (ADDED to), dgamma, dbeta; two launches (the pass over g / x1 / x, and the combination of the workgroups' slabs in `ws`), always
 * bit-reproducible.  Replaces salsa_nn_bn_bwd(dx = NULL) + salsa_nn_conv3x3_stem_wrw_bn: one pass over g and x1 instead of two. */
extern "C" int salsa_nn_conv3x3_stem_wrw_bnf(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *g,
                                             const void *x1, const float *mean, const float *invstd, const float *gamma,
                                             const float *beta, int relu, float *dw, float *dgamma, float *dbeta, void *ws,
                                             size_t ws_bytes, int64_t N, int Cin, int H, int W, void *hip_stream)
{
    if (!x || !g || !x1 || !mean || !invstd || !gamma || !beta || !dw || !dgamma || !dbeta || !ws || N <= 0 || Cin <= 0 || Cin > 14 ||
        H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH || x_channel_stride < (int64_t)H * W || x_batch_stride < x_channel_stride * Cin ||
        x_channel_stride * Cin >= INT32_MAX)
        return -1;
    const long tiles = (long)N * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W);
    const StemBnf bnf = {mean, invstd, gamma, beta};
    hipStream_t st = (hipStream_t)hip_stream;
    if (Cin > 7) {
        if (ws_bytes < salsa_nn_conv3x3_stem16_wrw_bnf_ws_bytes(N, H, W)) return -5;
        const unsigned nb = (unsigned)(tiles >= STEM16_WRW_BN_GRID ? STEM16_WRW_BN_GRID : tiles);
        hipLaunchKernelGGL((conv3x3_stem_wrw_kernel<2, 2>), dim3(nb), dim3(256), 0, st, x, (long)x_batch_stride, (long)x_channel_stride,
                           (const unsigned short *)g, dw, (int)N, Cin, H, W, (const unsigned short *)x1, (const float *)nullptr, relu,
                           (float *)ws, bnf);
        hipLaunchKernelGGL(stem_wrw_bnf_finalize_kernel<2>, dim3(64), dim3(1024), 0, st, (const float *)ws, (int)nb, (double)(N * H * W),
                           Cin * 9, bnf, dw, dgamma, dbeta);
        return hipGetLastError() == hipSuccess ? 0 : -6;
    }
    if (ws_bytes < salsa_nn_conv3x3_stem_wrw_bnf_ws_bytes(N, H, W)) return -5;
    const unsigned nb = (unsigned)(tiles >= STEM_WRW_BN_GRID ? STEM_WRW_BN_GRID : tiles);
    hipLaunchKernelGGL(conv3x3_stem_wrw_kernel<2>, dim3(nb), dim3(256), 0, st, x, (long)x_batch_stride, (long)x_channel_stride,
                       (const unsigned short *)g, dw, (int)N, Cin, H, W, (const unsigned short *)x1, (const float *)nullptr, relu,
                       (float *)ws, bnf);
    hipLaunchKernelGGL(stem_wrw_bnf_finalize_kernel<1>, dim3(64), dim3(1024), 0, st, (const float *)ws, (int)nb, (double)(N * H * W), Cin * 9,
                       bnf, dw, dgamma, dbeta);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// The same with the BatchNorm (+ ReLU) that follows the first layer differentiated on the fly: g = gradient of the BatchNorm's
// OUTPUT, x1 = its input (the first layer's output), both bf16 channels-last; coef = the [7][64] table salsa_nn_bn_bwd leaves in
// coef_ws (call it with dx = NULL: it then skips its apply pass, whose only reader would have been this kernel).
extern "C" int salsa_nn_conv3x3_stem_wrw_bn(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *g,
                                            const void *x1, const float *coef, int relu, float *dw, int64_t N, int Cin, int H, int W,
                                            void *hip_stream)
{
    if (!x || !g || !x1 || !coef || !dw || N <= 0 || Cin <= 0 || Cin > 14 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH ||
        x_channel_stride < (int64_t)H * W || x_batch_stride < x_channel_stride * Cin ||
        x_channel_stride * Cin >= INT32_MAX /* 32-bit element offsets inside an image */)
        return -1;
    const long tiles = (long)N * ((H + WT_H - 1) / WT_H) * ((W + WT_W - 1) / WT_W);
    // persistent; this instantiation holds 246 registers (two sets of tile loads in flight): TWO workgroups per CU are resident, so
    // the grid is a whole number of rounds of 512 (1280 left the last half round on half the CUs)
    const unsigned nb = (unsigned)(tiles >= STEM_WRW_BN_GRID ? STEM_WRW_BN_GRID : tiles);
    int rc = 0;
    float *part = salsa_nn_det_begin((int)nb, 64L * Cin * 9, (hipStream_t)hip_stream, &rc);
    if (rc) return rc;
    hipLaunchKernelGGL((Cin <= 7 ? conv3x3_stem_wrw_kernel<1> : conv3x3_stem_wrw_kernel<1, 2>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, x, (long)x_batch_stride,
                       (long)x_channel_stride, (const unsigned short *)g, dw, (int)N, Cin, H, W, (const unsigned short *)x1, coef, relu, part, StemBnf{});
    if (part) return salsa_nn_det_finish(part, (int)nb, 64L * Cin * 9, dw, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
