// conv_mfma.hip -- 3x3 / stride 1 / pad 1 convolution, 64 -> 64 channels, channels-last bf16, on the gfx950 matrix cores.
// Implicit GEMM computed transposed, C^T[co][pixel] = sum_{tap,ci} W[tap][co][ci] * X[pixel+tap][ci], so that
//   A (32 co x 16 ci)     = 16 contiguous bytes of the weight row [co][ci..ci+7]       per lane (lane&31 = co, lane>>5 = k half)
//   B (16 ci x 32 pixels) = 16 contiguous bytes of the input pixel [pixel][ci..ci+7]    per lane (lane&31 = pixel)
//   D (32 co x 32 pixels) = for ONE pixel per lane, 4 groups of 4 consecutive co        -> 8-byte bf16 stores
// i.e. neither operand needs a transpose and the result is written pixel-major (NHWC) with vector stores.
// A persistent workgroup (4 waves) walks output tiles of 4 rows x 32 pixels: wave = one half of the output channels x one
// pair of rows, its slice of the filter (9 taps x 32 co x 64 ci bf16 = 36 fragments) held in REGISTERS for the whole launch;
// only the input halo tile goes through LDS (rows padded 128 -> 144 bytes so the 16-byte operand reads of 32 consecutive
// pixels spread over all banks), the next tile's loads in flight during the current tile's MFMAs.
// The first layer's kernel is conv_stem.hip, the weight gradients are conv_c64_wrw.hip and conv_stem_wrw.hip; what they share
// with this file (operand types, tile geometry, the statistics sums, the XCD walk, the launch plan) is conv_internal.h.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include "conv_internal.h"

namespace {

#ifndef CONV_WIDE_STORE
#define CONV_WIDE_STORE 1 // 16-byte epilogue stores through v_permlane32_swap (0: the 8-byte stores of rounds 1-2)
#endif
#ifndef CONV64_OUT_NT
#define CONV64_OUT_NT 0 // round-5 probe: the plain epilogue's 16-byte output stores as non-temporal stores (written once; the input's halo rows are what the L2 should keep)
#endif
#ifndef CONV_WPS
#define CONV_WPS 2
#endif
constexpr int HALO_PIECES = HALO_H * HALO_W * 8;              // 16-byte pieces of one input tile
constexpr int PREF = (HALO_PIECES + 255) / 256;               // pieces per thread

// x: [N][H][W][64] bf16, w: [64 co][3][3][64 ci] bf16 (torch's channels-last weight layout), y: [N][H][W][64] bf16.
// Epilogue of one tile, shared by the two forward kernels: D -> (shift, residual, ReLU) -> bf16 stores, or the pooled variant.
template <bool POOL>
__device__ __forceinline__ void conv64_epilogue(const f32x16 (&acc)[RPW], unsigned short *__restrict__ y, const float *__restrict__ shift,
                                                const float4 (&shv)[4], const unsigned short *__restrict__ residual, int relu, long n,
                                                int th, int tw, int H, int W, int lane, int px, int mb, int rg, const Geo &geo,
                                                const uint2 (*pre)[4] = nullptr /* RES: the tile's residual pieces, loaded at the tile's top */)
{
    if (POOL) { // inference, RPW == 2: the 2x2 average pool that follows (stem, model_utils.py:224) taken on the float32 values
        // before the single rounding -- the wave's two rows are the vertical pair, the neighbouring lane the horizontal one;
        // the full-resolution activation is never written (H and W even: a tile holds whole 2x2 cells)
        const int h0 = th * TH + rg * RPW, wcol = tw * TW + px;
        const bool inside = h0 < H && wcol < W;
        uint2 pk[4];
        uint2 rvp[RPW][4];
        if (residual && pre) {
#pragma unroll
            for (int rr = 0; rr < RPW; rr++)
#pragma unroll
                for (int g = 0; g < 4; g++) rvp[rr][g] = pre[rr][g];
        } else if (residual) { // (all eight pieces requested together: see the plain epilogue below)
#pragma unroll
            for (int rr = 0; rr < RPW; rr++) {
                const long roff = geo_off(geo, n, inside ? h0 + rr : 0, inside ? wcol : 0) + 32 * mb + 4 * (lane >> 5);
#pragma unroll
                for (int g = 0; g < 4; g++) rvp[rr][g] = *(const uint2 *)(residual + roff + 8 * g);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            float s4[4] = {0.f, 0.f, 0.f, 0.f};
            const float4 sh = shv[g];
#pragma unroll
            for (int rr = 0; rr < RPW; rr++) {
                float v4[4] = {acc[rr][4 * g] + sh.x, acc[rr][4 * g + 1] + sh.y, acc[rr][4 * g + 2] + sh.z, acc[rr][4 * g + 3] + sh.w};
                if (residual) {
                    const uint2 rv = rvp[rr][g];
                    v4[0] += __uint_as_float(rv.x << 16); v4[1] += __uint_as_float(rv.x & 0xffff0000u);
                    v4[2] += __uint_as_float(rv.y << 16); v4[3] += __uint_as_float(rv.y & 0xffff0000u);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) s4[j] += relu ? fmaxf(v4[j], 0.f) : v4[j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) s4[j] = 0.25f * (s4[j] + __shfl_xor(s4[j], 1));
            pk[g].x = pack_bf16(s4[0], s4[1]);
            pk[g].y = pack_bf16(s4[2], s4[3]);
        }
        // 16-byte stores: runs traded with the partner lane (same pixel, lane +- 32), as in the plain epilogue below
        unsigned short *o = y + (n * geo.psn + (long)(inside ? h0 / 2 : 0) * geo.psh + (long)(inside ? wcol / 2 : 0) * geo.psw) + 32 * mb + 8 * (lane >> 5);
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            const auto sx = __builtin_amdgcn_permlane32_swap(pk[g].x, pk[g + 1].x, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(pk[g].y, pk[g + 1].y, false, false);
            if (inside && !(px & 1)) *(uint4 *)(o + 8 * g) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
        }
        return;
    }
    // A lane holds, of its pixel, four runs of 4 consecutive channels (8 g + 4 khalf + 0..3) and its partner lane (the same
    // pixel, lane +- 32) the other half of each 8-channel run.  Written as they lie that is four 8-byte stores per row: the
    // epilogue was store-ISSUE-bound (probe builds, 8 x 2400 x 100: 0.229 ms, 0.148 without the epilogue and its stores).
    // v_permlane32_swap (gfx950) trades runs between the two lanes -- the low lane gives away its runs 1 and 3 for the partner's
    // halves of runs 0 and 2 -- so that every lane owns two whole 8-channel runs: two 16-byte stores per row (round 3).
#pragma unroll
    for (int rr = 0; rr < RPW; rr++) {
        const int h = th * TH + rg * RPW + rr, wcol = tw * TW + px;
        const bool inside = h < H && wcol < W;      // (the same for both lanes of a pair: they share the pixel)
        const long off = geo_off(geo, n, inside ? h : 0, inside ? wcol : 0) + 32 * mb + 4 * (lane >> 5);
        uint2 pk[4];
        // (round 4: the row's four residual pieces are requested together -- fetched inside the g loop the compiler waited
        // `vmcnt(0)` after each one: four dependent round trips per row, in inference and in the data gradients that add a skip branch)
        uint2 rvq[4] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
        if (shift && residual && pre) {
#pragma unroll
            for (int g = 0; g < 4; g++) rvq[g] = pre[rr][g];
        } else if (shift && residual) {
#pragma unroll
            for (int g = 0; g < 4; g++) rvq[g] = *(const uint2 *)(residual + off + 8 * g);
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            float v4[4] = {acc[rr][4 * g], acc[rr][4 * g + 1], acc[rr][4 * g + 2], acc[rr][4 * g + 3]};
            if (shift) { // inference epilogue: folded BatchNorm shift (+ residual) (+ ReLU) before the single rounding
                const float4 sh = shv[g];
                v4[0] += sh.x; v4[1] += sh.y; v4[2] += sh.z; v4[3] += sh.w;
                if (residual) {
                    const uint2 rv = rvq[g];
                    v4[0] += __uint_as_float(rv.x << 16); v4[1] += __uint_as_float(rv.x & 0xffff0000u);
                    v4[2] += __uint_as_float(rv.y << 16); v4[3] += __uint_as_float(rv.y & 0xffff0000u);
                }
                if (relu) {
#pragma unroll
                    for (int j = 0; j < 4; j++) v4[j] = fmaxf(v4[j], 0.f);
                }
            }
            pk[g].x = pack_bf16(v4[0], v4[1]);
            pk[g].y = pack_bf16(v4[2], v4[3]);
        }
#if CONV_WIDE_STORE
        // swap(A, B): lanes 32-63 of A <-> lanes 0-31 of B.  With A = run g (even), B = run g + 1: the low lane ends with
        // (own half of run g, partner's half of run g) = channels 8 g .. 8 g + 7, the high lane with the two halves of run g + 1
        unsigned short *o = y + geo_off(geo, n, inside ? h : 0, inside ? wcol : 0) + 32 * mb + 8 * (lane >> 5);
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
            const auto sx = __builtin_amdgcn_permlane32_swap(pk[g].x, pk[g + 1].x, false, false);
            const auto sy = __builtin_amdgcn_permlane32_swap(pk[g].y, pk[g + 1].y, false, false);
            const uint4 v = make_uint4(sx[0], sy[0], sx[1], sy[1]);
#ifdef CONV_NO_STORE // probe: everything computed, nothing written
            if (v.x == 0x12345678u && v.y == 0x9abcdef0u)
#endif
            if (inside) {
#if CONV64_OUT_NT
                typedef unsigned u4v_t __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(u4v_t{v.x, v.y, v.z, v.w}, (u4v_t *)(o + 8 * g));
#else
                *(uint4 *)(o + 8 * g) = v;
#endif
            }
        }
#else
        if (inside) {
            unsigned short *o = y + off;
#pragma unroll
            for (int g = 0; g < 4; g++) {
#ifdef CONV_NO_STORE
                if (pk[g].x == 0x12345678u && pk[g].y == 0x9abcdef0u)
#endif
                *(uint2 *)(o + 8 * g) = pk[g];
            }
        }
#endif
    }
}

// The WHOLE filter lives in registers (72 A fragments per lane: a wave per SIMD may use all 512 VGPR+AGPR), so LDS only
// serves the input tile: one 16-byte B read per two MFMAs.  The next tile's halo is prefetched into registers while the
// current tile is multiplied.
template <bool POOL>
__global__ __launch_bounds__(256, CONV_WPS) void conv3x3_c64_fwd_kernel(const unsigned short *__restrict__ x,
                                                              const unsigned short *__restrict__ w,
                                                              unsigned short *__restrict__ y, int N, int H, int W,
                                                              const float *__restrict__ shift,
                                                              const unsigned short *__restrict__ residual, int relu,
                                                              double *__restrict__ /* statistics: the LDS-direct kernel only */)
{
    __shared__ __attribute__((aligned(16))) unsigned short xl[HALO_H * HALO_W * ROW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 31, kh = (lane >> 5) * 8;
    const int mb = wv & 1, rg = wv >> 1; // this wave: output channels 32*mb .. +31, tile rows RPW*rg .. +RPW-1
    bf16x8 af[9][4];    // [tap][16-channel step]: filter row co = 32*mb + (lane&31), input channels kc*16 + kh .. +7
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int kc = 0; kc < 4; kc++) af[tap][kc] = *(const bf16x8 *)(w + ((long)((mb * 32 + px) * 9 + tap) * CH + kc * 16 + kh));
    float4 shv[4]; // the lane's 16 folded-BatchNorm shifts (inference), loaded once: ordinary loads inside the tile loop would
                   // make the compiler drain every load in flight, the next tiles' included
#pragma unroll
    for (int g = 0; g < 4; g++) shv[g] = shift ? *(const float4 *)(shift + 32 * mb + 4 * (lane >> 5) + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int tiles_w = (W + TW - 1) / TW, tiles_h = (H + TH - 1) / TH;
    const long n_tiles = (long)N * tiles_h * tiles_w;
    uint4 pre[PREF];
    auto fetch = [&](long tile) {
        const int tw = (int)(tile % tiles_w);
        const int th = (int)((tile / tiles_w) % tiles_h);
        const long n = tile / ((long)tiles_w * tiles_h);
#pragma unroll
        for (int j = 0; j < PREF; j++) {
            const int i = tid + j * 256;
            const int piece = i & 7, p = i >> 3;
            const int hh = p / HALO_W, ww = p - hh * HALO_W;
            const int h = th * TH + hh - 1, wcol = tw * TW + ww - 1;
            pre[j] = make_uint4(0u, 0u, 0u, 0u);
#ifndef CONV_NO_FETCH // probe: what the kernel costs without its input stream
            if (i < HALO_PIECES && h >= 0 && h < H && wcol >= 0 && wcol < W)
                pre[j] = *(const uint4 *)(x + (((n * H + h) * W + wcol) * CH + piece * 8));
#endif
        }
    };
    long tile = blockIdx.x;
    if (tile < n_tiles) fetch(tile);
    for (; tile < n_tiles; tile += gridDim.x) {
        __syncthreads(); // the previous tile's LDS reads are done
#pragma unroll
        for (int j = 0; j < PREF; j++) {
            const int i = tid + j * 256;
            if (i < HALO_PIECES) *(uint4 *)(xl + (long)(i >> 3) * ROW + (i & 7) * 8) = pre[j];
        }
        __syncthreads();
        if (tile + gridDim.x < n_tiles) fetch(tile + gridDim.x); // in flight during the multiply below
        const int tw = (int)(tile % tiles_w);
        const int th = (int)((tile / tiles_w) % tiles_h);
        const long n = tile / ((long)tiles_w * tiles_h);
        f32x16 acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; r++) acc[r] = f32x16{};
        // 36 K-steps (9 taps x 4 channel blocks), software-pipelined BY HAND: the compiler sinks plain LDS loads down to their
        // first use (ds_read ; s_waitcnt ; mfma), which leaves the matrix pipe idle for the LDS latency every step.  So the
        // B reads are volatile asm with the step's constant byte offset as the instruction's immediate, and the wait is an
        // asm that takes the fragments as operands: step q+1's fragments are requested, step q's four MFMAs issue, then wait.
        const unsigned lbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)xl +
                               2u * (unsigned)((rg * RPW * HALO_W + px) * ROW + kh);
#if CONV_RPW == 2 && !defined(CONV_NO_ROW_SHARE)
        // Output rows 0 and 1 of the wave read input rows 0-2 and 1-3: a fragment of input row ir (tap column s, channel block
        // kc) serves output row 0 with filter row ir and output row 1 with filter row ir-1.  Walking the 4 x 3 x 4 = 48 distinct
        // fragments instead of the 2 x 36 (row, step) pairs cuts the LDS reads by a third for the same 72 MFMAs (the LDS pipe,
        // shared by the CU's 8 waves, was as busy as the matrix pipe).
#define LDS_B1(dst, u)                                                                                                 \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                                                       \
                 : "=v"(dst)                                                                                           \
                 : "v"(lbase), "n"(2 * ((((u) / 12) * HALO_W + ((u) / 4) % 3) * ROW + ((u) & 3) * 16)))
#define LDS_WAIT1(f) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f))
#ifndef CONV_DEPTH
#define CONV_DEPTH 1 // fragments in flight ahead of the one being multiplied (1, 2, 3 measured the same)
#endif
        constexpr int DEPTH = CONV_DEPTH, RING = DEPTH + 1;
        bf16x8 bb[RING]; // fragment u multiplies while u+1 .. u+DEPTH are in flight (one MFMA pair is shorter than the LDS latency)
#pragma unroll
        for (int u = 0; u < DEPTH; u++) LDS_B1(bb[u % RING], u);
#pragma unroll
        for (int u = 0; u < 48; u++) {
            if (u + DEPTH < 48) LDS_B1(bb[(u + DEPTH) % RING], u + DEPTH);
            // wait until fragment u has landed: at most min(DEPTH, 47 - u) younger reads may still be outstanding
            if (u + DEPTH < 48) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(bb[u % RING]) : "n"(DEPTH));
            else if (47 - u == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(bb[u % RING]));
            else if (47 - u == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(bb[u % RING]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bb[u % RING]));
            __builtin_amdgcn_sched_barrier(0);
            const int ir = u / 12, sx = (u / 4) % 3, kc = u & 3;
            if (ir <= 2) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ir * 3 + sx][kc], bb[u % RING], acc[0], 0, 0, 0);
            if (ir >= 1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[(ir - 1) * 3 + sx][kc], bb[u % RING], acc[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
#undef LDS_B1
#undef LDS_WAIT1
#else
#define LDS_B(dst, q, rr)                                                                                              \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                                                       \
                 : "=v"(dst)                                                                                           \
                 : "v"(lbase), "n"(2 * ((((rr) + ((q) >> 2) / 3) * HALO_W + ((q) >> 2) % 3) * ROW + ((q) & 3) * 16)))
#if CONV_RPW == 4
#define LDS_WAIT(f) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]))
#else
#define LDS_WAIT(f) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]))
#endif
        bf16x8 bb[2][RPW]; // ping-pong: step q multiplies bb[q&1] while bb[(q+1)&1] is in flight
#pragma unroll
        for (int rr = 0; rr < RPW; rr++) LDS_B(bb[0][rr], 0, rr);
        LDS_WAIT(bb[0]);
#pragma unroll
        for (int q = 0; q < 36; q++) {
            if (q + 1 < 36) {
#pragma unroll
                for (int rr = 0; rr < RPW; rr++) LDS_B(bb[(q + 1) & 1][rr], q + 1, rr);
            }
            __builtin_amdgcn_sched_barrier(0); // the four reads go out BEFORE this step's MFMAs (which then cover their latency)
#pragma unroll
            for (int rr = 0; rr < RPW; rr++) acc[rr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[q >> 2][q & 3], bb[q & 1][rr], acc[rr], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 1 < 36) LDS_WAIT(bb[(q + 1) & 1]);
        }
#undef LDS_B
#undef LDS_WAIT
#endif
        // D: column = lane&31 = pixel, row (= co within this wave's 32) = (reg&3) + 8*(reg>>2) + 4*(lane>>5): a lane holds, for ONE
        // pixel, four groups of four consecutive output channels -> 8-byte stores.  (Transposing through a wave-private LDS
        // strip to get 16-byte stores of 64 contiguous bytes per pixel was measured SLOWER here, 1.59 -> 2.03 ms per training
        // step, twice: this kernel's epilogue competes with the next tile's MFMAs for LDS and registers.  The stem kernel
        // below, which has next to no MFMA work, does gain from it.)
        conv64_epilogue<POOL>(acc, y, shift, shv, residual, relu, n, th, tw, H, W, lane, px, mb, rg,
                              Geo{(long)H * W * CH, W * CH, CH, 0, (long)(H / 2) * (W / 2) * CH, (W / 2) * CH, CH});
    }
}

// ---- variant with the input tiles loaded STRAIGHT INTO LDS (global_load_lds_dwordx4), two tiles ahead.
// Probe builds of the kernel above: 0.242 ms for 8 x 2400 x 100, 0.143 ms without its input loads -- the next tile's halo,
// prefetched into registers ONE tile ahead, arrives later than one tile's multiply takes, and 256 VGPRs leave no room for a
// second staging set.  Direct-to-LDS loads need no staging registers: three LDS tiles (2 x 78 KB per CU) rotate, the loads
// for tile i+2 are issued when tile i starts, and the LDS write pass and one of the two barriers per tile disappear.  A wave's
// load instruction fills 64 consecutive 16-byte LDS slots, so the pixel stride in LDS is exactly 128 bytes; the bank
// conflicts that the padded layout avoided are avoided here by a rotation: channel block c of pixel p sits in slot
// (c + p) & 7, applied to the GLOBAL address when loading and to the LDS address when reading (where pixel and block offsets
// of a fragment are compile-time constants: eight per-lane base registers, one per value of the constant part mod 8).  Halo pixels outside the
// image load from a 16-byte zero constant.
__device__ uint4 conv_zero16; // zero-initialised
// its address pinned in a scalar register pair (used in place it is re-loaded from the GOT -- s_getpc, s_load_dwordx2, s_waitcnt
// lgkmcnt(0) -- in front of the halo loads of every tile; see conv_wide.hip wide_zero_ptr)
__device__ __forceinline__ const unsigned short *conv_zero_ptr()
{
    const unsigned short *z = (const unsigned short *)&conv_zero16;
    asm volatile("" : "+s"(z));
    return z;
}

constexpr int APIX = 64;                             // bf16 per pixel in LDS (no padding)
constexpr int ABUF = HALO_H * HALO_W * APIX;         // one tile
constexpr int NBUF = 3;
constexpr int AFETCH = (HALO_PIECES + 255) / 256;    // load instructions per thread per tile (the last one partial)

// The 48 fragment steps of one tile of the LDS-direct kernel as a compile-time recursion (every index a constant: written as a
// loop over a permuted step number the filter array was indexed "dynamically" and the compiler moved it to scratch memory).
// Step S multiplies fragment FRAG(S) = (input row ir, tap column sx, channel block kc) while the next AD fragments are in
// flight; rb[] are the lane's eight rotated base addresses (see the kernel).
#ifndef CONV_FETCH_NO_HOIST
#define CONV_FETCH_NO_HOIST 1
#endif
#ifndef CONV_RES_EARLY
#define CONV_RES_EARLY 1
#endif
#ifndef CONV_ORDER
#define CONV_ORDER 1 // 1: fragments ordered so that consecutive MFMAs never share an accumulator (0: row by row, round 1)
#endif
constexpr int conv64_frag(int s) { return CONV_ORDER ? (s < 24 ? ((s & 1) ? 36 + (s >> 1) : (s >> 1)) : 12 + (s - 24)) : s; }

template <int U>
__device__ __forceinline__ void conv64_lds_read(bf16x8 &dst, const unsigned (&rb)[8])
{
    constexpr int ir = U / 12, sx = (U / 4) % 3, kc = U & 3;
#ifdef CONV_NO_LDSREAD // probe: the fragment is whatever the register holds
    asm volatile("" : "=v"(dst) : "v"(rb[(2 * kc + sx + 2 * ir) & 7]));
#else
    asm volatile("ds_read_b128 %0, %1 offset:%2"
                 : "=v"(dst)
                 : "v"(rb[(2 * kc + sx + 2 * ir) & 7]), "n"(2 * ((ir * (TW + 2) + sx) * 64)));
#endif
}

#ifdef CONV_NO_SCHED // (probe: let the compiler order the step stream)
#define CONV_SCHED_BARRIER() do {} while (0)
#else
#define CONV_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#endif
// HOOK: called with std::integral_constant<int, j> before step CONV_HOOK_FIRST + CONV_HOOK_EVERY * j, j = 0 .. AFETCH - 1: the
// kernel issues one wave-load of the tile-after-next there (see "spread fetch" in the kernel)
#ifndef CONV_HOOK_FIRST
#define CONV_HOOK_FIRST 2
#endif
#ifndef CONV_HOOK_EVERY
#define CONV_HOOK_EVERY 6
#endif
struct conv64_no_hook {
    template <class J> __device__ __forceinline__ void operator()(J) const {}
};
template <int S, int AD, class HOOK = conv64_no_hook>
__device__ __forceinline__ void conv64_steps(const bf16x8 (&af)[9][4], bf16x8 (&bb)[AD + 1], f32x16 (&acc)[RPW], const unsigned (&rb)[8],
                                             const HOOK &hook = HOOK())
{
    constexpr int RING = AD + 1;
    if constexpr (S >= CONV_HOOK_FIRST && (S - CONV_HOOK_FIRST) % CONV_HOOK_EVERY == 0 && (S - CONV_HOOK_FIRST) / CONV_HOOK_EVERY < 8 && S < 48)
        hook(std::integral_constant<int, (S - CONV_HOOK_FIRST) / CONV_HOOK_EVERY>{});
    if constexpr (S == 0) {
#pragma unroll
        for (int s = 0; s < AD; s++) { // (AD is 1 or 2: spelled out so that the fragment numbers stay template constants)
            if (s == 0) conv64_lds_read<conv64_frag(0)>(bb[0], rb);
            if (s == 1) conv64_lds_read<conv64_frag(1)>(bb[1 % RING], rb);
            if (s == 2) conv64_lds_read<conv64_frag(2)>(bb[2 % RING], rb);
        }
    }
    if constexpr (S < 48) {
        if constexpr (S + AD < 48) conv64_lds_read<conv64_frag(S + AD < 48 ? S + AD : 0)>(bb[(S + AD) % RING], rb);
        // fragment S has landed when at most the younger reads are outstanding
        if constexpr (S + AD < 48) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(bb[S % RING]) : "n"(AD));
        else if constexpr (47 - S == 2) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(bb[S % RING]));
        else if constexpr (47 - S == 1) asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(bb[S % RING]));
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bb[S % RING]));
        CONV_SCHED_BARRIER();
        constexpr int u = conv64_frag(S), ir = u / 12, sx = (u / 4) % 3, kc = u & 3;
        // (the first product into each accumulator takes a ZERO C operand -- an inline constant of the instruction -- instead of
        // 32 v_mov clearing the accumulators every tile; with CONV_ORDER these are steps 0 (row 0 -> acc 0) and 1 (row 3 -> acc 1))
        constexpr bool first0 = CONV_ORDER && S == 0, first1 = CONV_ORDER && S == 1;
        if constexpr (ir <= 2) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ir * 3 + sx][kc], bb[S % RING], first0 ? f32x16{} : acc[0], 0, 0, 0);
        if constexpr (ir >= 1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[(ir - 1) * 3 + sx][kc], bb[S % RING], first1 ? f32x16{} : acc[1], 0, 0, 0);
        CONV_SCHED_BARRIER();
        conv64_steps<S + 1, AD, HOOK>(af, bb, acc, rb, hook);
    }
}

// RES (round 5): the launch adds a residual (inference: the block's shortcut; training: the skip branch's gradient in a data
// gradient).  Loaded inside the epilogue, the residual pieces were YOUNGER than the LDS-direct loads of the tile after next, so the
// `s_waitcnt vmcnt(0)` in front of their first use drained that prefetch and exposed the residual's own latency twice per tile (once
// per output row).  Here the tile's eight pieces are requested at the tile's TOP, before the prefetch is issued: they are older,
// the counted wait that lets the prefetch stay in flight covers them, and they land during the multiply.  16 registers, which
// the instantiation has once the load offsets are recomputed per tile (CONV_FETCH_NO_HOIST).
template <bool POOL, bool STATS = false, bool XF = false, bool RES = false>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_fwd_async_kernel(const unsigned short *__restrict__ x,
                                                                       const unsigned short *__restrict__ w,
                                                                       unsigned short *__restrict__ y, int N, int H, int W,
                                                                       const float *__restrict__ shift,
                                                                       const unsigned short *__restrict__ residual, int relu,
                                                                       double *__restrict__ stats_part, const Geo geo,
                                                                       const XformArgs xf = XformArgs{})
{
    static_assert(RPW == 2, "row sharing below is written for two rows per wave");
    static_assert(!(POOL && STATS), "statistics are a training feature, the fused pool an inference one");
    __shared__ __attribute__((aligned(16))) unsigned short xl[NBUF * ABUF];
    __shared__ float lstats[STATS ? 2 * 128 : 1]; // [row-group wave][sum | sum of squares][64 channels], used once after the last tile
    __shared__ __attribute__((aligned(16))) float xtab[XF ? 2 * 64 : 4]; // XF: scale[64] = invstd * gamma, shift[64] = beta - mean * scale
    float rs[4] = {0.f, 0.f, 0.f, 0.f}, rq[4] = {0.f, 0.f, 0.f, 0.f}; // STATS: this lane's running sums (conv64_stats)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (XF) {
        if (tid < 64) {
            const float sc = xf.invstd[tid] * xf.gamma[tid];
            xtab[tid] = sc;
            xtab[64 + tid] = xf.beta[tid] - xf.mean[tid] * sc;
        }
        __syncthreads(); // (before any LDS-direct load is in flight)
    }
    const int px = lane & 31, khalf = lane >> 5, kh = khalf * 8;
    const int mb = wv & 1, rg = wv >> 1;
    const unsigned short *const zero16 = conv_zero_ptr();
    bf16x8 af[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int kc = 0; kc < 4; kc++) // (transposed geometry: tap (ky, kx) multiplies the filter's (kx, ky))
            af[tap][kc] = *(const bf16x8 *)(w + ((long)((mb * 32 + px) * 9 + (geo.tap_t ? (tap % 3) * 3 + tap / 3 : tap)) * CH + kc * 16 + kh));
    float4 shv[4]; // the lane's 16 folded-BatchNorm shifts (inference), loaded once: ordinary loads inside the tile loop would
                   // make the compiler drain every load in flight, the next tiles' included
#pragma unroll
    for (int g = 0; g < 4; g++)
        shv[g] = (!STATS && shift) ? *(const float4 *)(shift + 32 * mb + 4 * (lane >> 5) + 8 * g) : make_float4(0.f, 0.f, 0.f, 0.f);

    // the filter has landed BEFORE the tile loop: left to its first use, the compiler's wait for these ordinary loads sits in
    // front of the loop's first MFMA as vmcnt(0) and drains the LDS-direct loads in flight with it, every tile
#pragma unroll
    for (int tap = 0; tap < 9; tap++)
#pragma unroll
        for (int kc = 0; kc < 4; kc++) asm volatile("" ::"v"(af[tap][kc]));
#pragma unroll
    for (int g = 0; g < 4; g++) asm volatile("" ::"v"(shv[g].x), "v"(shv[g].y), "v"(shv[g].z), "v"(shv[g].w));
    const int tiles_w = (W + TW - 1) / TW, tiles_h = (H + TH - 1) / TH;
    // Tile cursors.  Probe builds with neither loads nor stores still ran at 2x the MFMA time: the per-tile integer work
    // (two divisions per decode, a division by 34 and 64-bit address arithmetic per load) was the bound.  So a cursor keeps
    // (tw, th, n) and steps by the grid size with carries, and a thread's halo pixel walks rows incrementally (its channel
    // block never changes: the slot index advances by 256 = 0 mod 8 and the pixel by 32 = 0 mod 8 per load).
    struct Cursor { int tw, th, n; };
    const TileWalk walk = tile_walk(N, tiles_h, tiles_w, (int)gridDim.x, (int)blockIdx.x);
    const int stride = walk.G;                       // step of this workgroup's position in its XCD's tile sequence
    auto cursor_of = [&](const TilePos &p) {
        Cursor c;
        c.tw = p.tw;
        tile_coords(walk, p, c.n, c.th);
        return c;
    };
    const int p0 = tid >> 3, hh0 = p0 / HALO_W, ww0 = p0 - hh0 * HALO_W;
    const int blk8 = (((tid & 7) - p0) & 7) * 8; // channel offset of this thread's 16 bytes: slot (block + pixel) & 7
    auto fetch = [&](const Cursor &c, int buf) {
        const unsigned short *origin = x + geo_off(geo, c.n, c.th * TH, c.tw * TW); // pixel (0, 0) of the tile
        const int h_lo = -c.th * TH, h_hi = H - c.th * TH, w_lo = -c.tw * TW, w_hi = W - c.tw * TW; // valid (row, col) - origin
        int hh = hh0 - 1, ww = ww0 - 1; // halo pixel relative to the tile origin
#if CONV_FETCH_NO_HOIST
        // Round 5.  hh0 / ww0 never change, so the compiler hoisted the seven pieces' sign-extended element offsets out of the tile
        // loop as seven 64-bit register pairs -- and in the instantiations that need a few registers more (the statistics epilogue:
        // 8 running sums) it SPILLED three of them: every tile then reloaded them from scratch with `s_waitcnt vmcnt(0)` in front of
        // the LDS-direct load that uses them, i.e. three times per tile a wave sat out everything it had in flight, the next two
        // tiles' loads included (+70 us on the 311-us kernel at 32 x 640 x 200; found in the ISA, the counters only showed
        // "waiting").  Laundering the two start values makes the offsets loop-variant: ~5 integer instructions per piece per tile,
        // recomputed, and nothing to spill.
        // (Only where it spilled: the plain forward / data-gradient instantiation fits with the offsets hoisted and is 2 - 7 % faster so.)
        if (STATS || POOL || XF || RES) asm volatile("" : "+v"(hh), "+v"(ww));
#endif
#pragma unroll
        for (int j = 0; j < AFETCH; j++) {
            const bool inside = hh >= h_lo && hh < h_hi && ww >= w_lo && ww < w_hi;
            const unsigned short *src = inside ? origin + (hh * geo.sh + ww * geo.sw + blk8) : zero16;
#ifdef CONV_ZERO_SRC // (probe: every halo load answered from one cached line)
            src = zero16;
#endif
#ifdef CONV_PROBE_ROLL // (TIMING probe, wrong results: two of the six halo rows answered from one cached line -- the traffic of a tile
            if (hh < 1) src = zero16; // walk that keeps the rows consecutive tiles share in LDS)
#endif
#ifdef CONV_FETCH_COLMAJOR // (TIMING probe, wrong results: neighbouring lanes fetch along the tile's SHORT axis -- contiguous 768-byte
            {              // runs in the transposed geometry -- instead of along the long one, 34 lines a map row apart)
                const int q = (tid >> 3) + 32 * j, h2 = q % HALO_H - 1, w2 = q / HALO_H - 1;
                const bool in2 = q < HALO_H * HALO_W && h2 >= h_lo && h2 < h_hi && w2 >= w_lo && w2 < w_hi;
                src = in2 ? origin + (h2 * geo.sh + w2 * geo.sw + blk8) : zero16;
            }
#endif
            unsigned short *dst = xl + buf * ABUF + (j * 256 + wv * 64) * 8; // the wave's 64 slots (lane l -> + 16 l bytes)
#ifndef CONV_NO_FETCH
            if (tid + j * 256 < HALO_PIECES)
#else
            if (tid < 0)
#endif
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
            ww += 32; // the next load of this thread: 32 pixels on
            const int wrap = ww >= HALO_W - 1 ? 1 : 0;
            ww -= wrap ? HALO_W : 0;
            hh += wrap;
        }
    };
    // Spread fetch (round 4 experiment, OFF).  Counters of this kernel at 32 x 640 x 200 (tools/probes/pmc_mem.sh): the CU's L1 is
    // stalled on pending requests 73 % of the launch and on its translation queue 30 %, while an L2 read is answered in ~800 cycles
    // on average; it sees 9.5e7 accesses per launch -- one per LANE of every 16-byte load and store, halo re-reads included -- i.e.
    // 373 k accesses per CU in a 551 k-cycle launch, and with every load answered from one cached line (CONV_ZERO_SRC) the same
    // accesses pass at 0.96 per cycle in 388 k cycles.  So the L1 path (about one 16-byte lane access per cycle and CU = 8 TB/s over
    // the chip) is this kernel's second roofline, next to the matrix pipe, and misses make each access dearer.  Hypothesis tested
    // here: the seven wave-loads of a tile, issued in one burst, block their waves in the ISSUE of the loads; so piece j of the
    // tile-after-next is issued from inside the multiply (conv64_steps' hook, address formed from the compile-time piece number).
    // Measured: plain forward 341 -> 349 us, with statistics 411 -> 399, 320 x 100 the same: it is the L1's RATE, not the burst.
#ifndef CONV_SPREAD_FETCH
#define CONV_SPREAD_FETCH 0
#endif
    struct FetchCtx { const unsigned short *origin; int h_lo, h_hi, w_lo, w_hi, buf; bool on; };
    auto fetch_ctx = [&](const Cursor &c, int buf, bool on) {
        FetchCtx f;
        f.origin = x + geo_off(geo, c.n, c.th * TH, c.tw * TW);
        f.h_lo = -c.th * TH; f.h_hi = H - c.th * TH; f.w_lo = -c.tw * TW; f.w_hi = W - c.tw * TW;
        f.buf = buf; f.on = on;
        return f;
    };
    auto fetch_piece = [&](auto jc, const FetchCtx &f) {
        constexpr int j = decltype(jc)::value;
        if constexpr (j < AFETCH) {
            if (f.on && (j * 256 + wv * 64 < HALO_PIECES)) { // (wave-uniform)
                const int q = p0 + 32 * j;                                    // this thread's halo pixel of piece j, row-major in 6 x 34
                const int hq = (q * 241) >> 13, wq = q - hq * HALO_W;         // q / 34 for q < 236
                const int hh = hq - 1, ww = wq - 1;
                const bool inside = hh >= f.h_lo && hh < f.h_hi && ww >= f.w_lo && ww < f.w_hi && tid + j * 256 < HALO_PIECES;
                const unsigned short *src = inside ? f.origin + (hh * geo.sh + ww * geo.sw + blk8) : zero16;
                unsigned short *dst = xl + f.buf * ABUF + (j * 256 + wv * 64) * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
            }
        }
    };
    static_assert(HALO_H * HALO_W + 31 < 236 && AFETCH <= 8, "q / 34 == (q * 241) >> 13; eight hook slots");
    // XF: rewrite this thread's own (landed) pieces of a tile in place
    auto transform = [&](const Cursor &c, int buf) {
        const int h_lo = -c.th * TH, h_hi = H - c.th * TH, w_lo = -c.tw * TW, w_hi = W - c.tw * TW;
        const long origin = geo_off(geo, c.n, c.th * TH, c.tw * TW); // element offset of the tile's pixel (0, 0) in the tensor
        const float4 s0 = *(const float4 *)(xtab + blk8), s1 = *(const float4 *)(xtab + blk8 + 4);
        const float4 t0 = *(const float4 *)(xtab + 64 + blk8), t1 = *(const float4 *)(xtab + 64 + blk8 + 4);
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, sh[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        int hh = hh0 - 1, ww = ww0 - 1;
#ifndef C64_XF_UNROLL
#define C64_XF_UNROLL 1 // pieces rewritten at a time: the filter owns the register file (unrolled by 7: 256 bytes of scratch per lane)
#endif
#pragma unroll C64_XF_UNROLL
        for (int j = 0; j < AFETCH; j++) {
            const bool inside = hh >= h_lo && hh < h_hi && ww >= w_lo && ww < w_hi;
            if (inside && tid + j * 256 < HALO_PIECES) {
                uint4 *slot = (uint4 *)(xl + buf * ABUF + (j * 256 + tid) * 8);
                const uint4 v = *slot;
                const unsigned in[4] = {v.x, v.y, v.z, v.w};
                unsigned out[4];
                const long e0 = origin + (long)hh * geo.sh + (long)ww * geo.sw + blk8; // the piece's first element in the tensor
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float a = fmaxf(__uint_as_float(in[k] << 16) * sc[2 * k] + sh[2 * k], 0.f);
                    float b = fmaxf(__uint_as_float(in[k] & 0xffff0000u) * sc[2 * k + 1] + sh[2 * k + 1], 0.f);
                    if (xf.drop.thresh) { // one 32-bit hash per pair of neighbouring elements, 16 bits each (drop_keep)
                        const unsigned hsh = drop_hash((unsigned)(e0 >> 1) + k, xf.drop.seed);
                        a = (hsh & 0xFFFFu) >= xf.drop.thresh ? a * xf.drop.scale : 0.f;
                        b = (hsh >> 16) >= xf.drop.thresh ? b * xf.drop.scale : 0.f;
                    }
                    out[k] = pack_bf16(a, b);
                }
                *slot = make_uint4(out[0], out[1], out[2], out[3]);
            }
            ww += 32;
            const int wrap = ww >= HALO_W - 1 ? 1 : 0;
            ww -= wrap ? HALO_W : 0;
            hh += wrap;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the rewritten pieces are in LDS before this wave reaches the next barrier
    };
    // Loads of ONE wave return in order, but its stores retire independently, so a counted wait is only exact where nothing
    // but loads is younger than the loads waited for.  Order per tile: barrier -> issue tile+2 -> multiply tile -> wait until
    // only tile+2's loads are outstanding (tile+1 has landed; the stores of the tile before retired during the multiply)
    // -> store tile.  The barrier then makes every wave's part of tile+1 visible and frees the buffer tile+3 goes into.
#define WAIT_ALL_BUT_LAST_FETCH()                                                        \
    do {                                                                                 \
        if (wv < (HALO_PIECES % 256 + 63) / 64) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AFETCH) : "memory");     \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AFETCH - 1) : "memory");             \
    } while (0)
    static_assert(HALO_PIECES % 256 != 0, "the last fetch instruction is issued by the first (HALO_PIECES % 256 + 63) / 64 waves only");
    const int n_tiles = walk.n_local;                // tiles of this workgroup's XCD; `tile` = position in that sequence
    int tile = (int)blockIdx.x / walk.nx;
    TilePos pcur = tile_pos(walk, tile), pahead = pcur;
    if (tile < n_tiles) fetch(cursor_of(pahead), 0);
    tile_advance(walk, pahead);
    TilePos pnext = pahead;                         // XF: one tile ahead of `pcur`
    if (tile + stride < n_tiles) {
        fetch(cursor_of(pahead), 1);
        WAIT_ALL_BUT_LAST_FETCH();
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (XF && tile < n_tiles) transform(cursor_of(pcur), 0);
    tile_advance(walk, pahead); // two tiles ahead of `pcur` from here on
    for (int it = 0; tile < n_tiles; tile += stride, it++, tile_advance(walk, pcur), tile_advance(walk, pahead), tile_advance(walk, pnext)) {
        const Cursor cur = cursor_of(pcur);
#ifndef CONV_NO_BARRIER // (probe)
        __builtin_amdgcn_s_barrier(); // (a raw barrier: __syncthreads() would drain the loads in flight)
#endif
        const int tw = cur.tw, th = cur.th;
        const long n = cur.n;
        uint2 rpre[RPW][4];
        if (RES) { // this tile's residual pieces, requested BEFORE the prefetch below (same addresses as conv64_epilogue's own loads)
#pragma unroll
            for (int rr = 0; rr < RPW; rr++) {
                const int h0 = th * TH + rg * RPW, wcol = tw * TW + px;
                const int h = POOL ? h0 + rr : h0 + rr;
                const bool inside = POOL ? (h0 < H && wcol < W) : (h < H && wcol < W);
                const unsigned short *rp = residual + (geo_off(geo, n, inside ? h : 0, inside ? wcol : 0) + 32 * mb + 4 * (lane >> 5));
                // (asm: as ordinary loads the compiler waits for them itself at their first use -- with `vmcnt(0)`, because the
                // prefetch behind them is issued conditionally and it merges the paths -- and drains the prefetch after all; the
                // counted wait after the multiply is what covers them)
                asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(rpre[rr][0]) : "v"(rp));
                asm volatile("global_load_dwordx2 %0, %1, off offset:16" : "=v"(rpre[rr][1]) : "v"(rp));
                asm volatile("global_load_dwordx2 %0, %1, off offset:32" : "=v"(rpre[rr][2]) : "v"(rp));
                asm volatile("global_load_dwordx2 %0, %1, off offset:48" : "=v"(rpre[rr][3]) : "v"(rp));
            }
        }
#if CONV_SPREAD_FETCH
        const FetchCtx fctx = fetch_ctx(cursor_of(pahead), (it + 2) % NBUF, tile + 2 * stride < n_tiles); // issued inside the multiply
#else
        if (tile + 2 * stride < n_tiles) fetch(cursor_of(pahead), (it + 2) % NBUF); // into the buffer of the tile before
#endif
        f32x16 acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; r++) acc[r] = f32x16{};
        // 48 distinct fragments (4 input rows x 3 tap columns x 4 channel blocks) for 72 MFMAs, as in the kernel above
        // fragment u = (input row ir, tap column sx, channel block kc): pixel (rg*RPW + ir) * 34 + px + sx, block 2*kc + khalf ->
        // slot (block + pixel) & 7 = (L + K) & 7 with L = the lane's part and K = 2*kc + sx + 2*ir (34 = 2 mod 8) compile-time
        unsigned rb[8];
        {
            const unsigned bbase = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned short *)xl +
                                   2u * (unsigned)((it % NBUF) * ABUF + (rg * RPW * HALO_W + px) * APIX);
            const int L = 2 * RPW * rg + px + khalf;
#pragma unroll
            for (int m = 0; m < 8; m++) rb[m] = bbase + 16u * (unsigned)((L + m) & 7);
        }
#define LDS_BA(dst, u)                                                                                                 \
    asm volatile("ds_read_b128 %0, %1 offset:%2"                                                                       \
                 : "=v"(dst)                                                                                           \
                 : "v"(rb[(2 * ((u) & 3) + ((u) / 4) % 3 + 2 * ((u) / 12)) & 7]), "n"(2 * ((((u) / 12) * HALO_W + ((u) / 4) % 3) * APIX)))
#ifndef CONV_ADEPTH
#define CONV_ADEPTH 1 // 1 and 2 measured the same, 3 slower (spills): LDS latency is not what this loop waits for
#endif
        constexpr int AD = CONV_ADEPTH, RING = AD + 1; // fragments in flight ahead of the one being multiplied
        bf16x8 bb[RING];
        // Fragment ORDER.  Input rows 0 and 3 serve one output row each, rows 1 and 2 both: walked row by row, the first and
        // the last 12 MFMAs of a tile all accumulate into the SAME register block back to back, and a dependent
        // v_mfma_f32_32x32x16_bf16 cannot start until its predecessor's 8 passes have drained (with the ds_read / s_waitcnt /
        // s_nop issue slots between them the gap is the microarchitecture guide's "+43 cycles" case): a third of the MFMAs
        // ran at half rate.  Interleaving row 0 with row 3 alternates the two accumulators on EVERY step.
#if CONV_SPREAD_FETCH
        conv64_steps<0, AD>(af, bb, acc, rb, [&](auto jc) { fetch_piece(jc, fctx); });
#else
        conv64_steps<0, AD>(af, bb, acc, rb);
#endif
#undef LDS_BA
        if (tile + 2 * stride < n_tiles) WAIT_ALL_BUT_LAST_FETCH();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (RES) // the residual pieces are older than everything the counted wait above lets stay in flight: they have landed
            asm volatile("" : "+v"(rpre[0][0]), "+v"(rpre[0][1]), "+v"(rpre[0][2]), "+v"(rpre[0][3]), "+v"(rpre[1][0]), "+v"(rpre[1][1]),
                              "+v"(rpre[1][2]), "+v"(rpre[1][3])
                         :: "memory");
#ifdef CONV_NO_EPI // probe: the accumulators are kept alive, nothing is converted or stored
        asm volatile("" ::"v"(acc[0]), "v"(acc[1]));
#else
        conv64_epilogue<POOL>(acc, y, STATS ? nullptr : shift, shv, residual, relu, n, th, tw, H, W, lane, px, mb, rg, geo, RES ? rpre : nullptr);
        if (STATS) conv64_stats(acc, rs, rq, th, tw, H, W, px, rg);
#endif
        // XF: tile i+1 -- this thread's pieces landed at the wait above; rewritten here, after the epilogue, where the accumulators
        // are dead (before it: 108 bytes of scratch per lane)
        if (XF && tile + stride < n_tiles) transform(cursor_of(pnext), (it + 1) % NBUF);
    }
#undef WAIT_ALL_BUT_LAST_FETCH
    if (STATS) { // this workgroup's partial sums: [2][64] float64, row blockIdx.x of the BatchNorm kernels' partial table
        // the 8 quads of a half-wave hold the same channel groups: three butterfly steps over pixel columns +4, +8, +16 (once per
        // launch; LDS atomics here cost 16 us of a 110-us launch), then the two row-group waves of a channel half meet in LDS
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int d = 4; d <= 16; d <<= 1) {
                rs[j] += __shfl_xor(rs[j], d);
                rq[j] += __shfl_xor(rq[j], d);
            }
        if (px < 4) {
            const int cbase = rg * 128 + 32 * mb + 4 * khalf + 8 * px;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                lstats[cbase + j] = rs[j];
                lstats[cbase + 64 + j] = rq[j];
            }
        }
        __syncthreads();
        if (tid < 128) stats_part[(long)blockIdx.x * 128 + tid] = (double)lstats[tid] + (double)lstats[128 + tid];
    }
}

#ifndef CONV_BIG_GRID
#define CONV_BIG_GRID 1024 // persistent workgroups for large inputs (two resident per CU)
#endif
#if CONV_ASYNC
#define CONV_FWD_KERNEL conv3x3_c64_fwd_async_kernel
#else
#define CONV_FWD_KERNEL conv3x3_c64_fwd_kernel
#endif

} // namespace

#if CONV_ASYNC
#define C64_GEO_ARG(pl) , (pl).geo
#else
#define C64_GEO_ARG(pl)
#endif

extern "C" int salsa_nn_conv3x3_c64(const void *x, const void *w, void *y, int64_t N, int H, int W, void *hip_stream)
{
    if (!x || !w || !y || x == y || N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH) return -1;
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    // persistent workgroups, two resident per CU: 512 or 1024 of them (multiples of 512 measured best), fewer for tiny inputs
    const unsigned nb = (unsigned)(pl.tiles >= 16384 ? CONV_BIG_GRID : pl.tiles >= 512 ? 512 : pl.tiles);
    hipLaunchKernelGGL(CONV_FWD_KERNEL<false>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned short *)x,
                       (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, (const float *)nullptr,
                       (const unsigned short *)nullptr, 0, (double *)nullptr C64_GEO_ARG(pl));
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

/* the forward plan: its tile count (TH x TW output pixels each), *transposed = the geometry's tap_t (see struct Geo); host only */
extern "C" int salsa_nn_conv3x3_c64_config(int64_t N, int H, int W, int *transposed)
{
    if (!transposed || N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH) return -1;
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    *transposed = pl.geo.tap_t;
    return (int)pl.tiles;
}

/* number of partial rows ([2][64] float64 each) salsa_nn_conv3x3_c64_stats writes = its workgroup count */
extern "C" int salsa_nn_conv3x3_c64_stats_blocks(int64_t N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH || !CONV_ASYNC) return 0;
    const long tiles = c64_plan(N, H, W, TH, TW).tiles;
    return (int)(tiles >= 16384 ? CONV_BIG_GRID : tiles >= 512 ? 512 : tiles);
}

// training: the plain convolution, which also leaves the per-channel sum / sum of squares of its (bf16-rounded) output as
// per-workgroup float64 partial rows stats_part[blocks][2][64] -- the BatchNorm that follows then needs no statistics pass
// over the tensor (salsa_nn_bn_train_fwd's stats_part / stats_blocks)
extern "C" int salsa_nn_conv3x3_c64_stats(const void *x, const void *w, void *y, double *stats_part, int64_t N, int H, int W,
                                          void *hip_stream)
{
    if (!x || !w || !y || !stats_part || x == y || !salsa_nn_conv3x3_c64_stats_blocks(N, H, W)) return -1;
    const unsigned nb = (unsigned)salsa_nn_conv3x3_c64_stats_blocks(N, H, W);
#if CONV_ASYNC
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    hipLaunchKernelGGL((conv3x3_c64_fwd_async_kernel<false, true>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream,
                       (const unsigned short *)x, (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, (const float *)nullptr,
                       (const unsigned short *)nullptr, 0, stats_part, pl.geo);
#endif
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// training, round 4: y = conv(a, w) with a = dropout(relu(batch_norm(x1))) formed on the fly from the RAW output x1 of the
// convolution before (XformArgs above) + the statistics epilogue of salsa_nn_conv3x3_c64_stats for the BatchNorm that follows
extern "C" int salsa_nn_conv3x3_c64_xform_stats(const void *x1, const void *w, void *y, double *stats_part, const float *mean,
                                                const float *invstd, const float *gamma, const float *beta, float drop_p,
                                                uint32_t drop_seed, int64_t N, int H, int W, void *hip_stream)
{
    if (!x1 || !w || !y || !stats_part || x1 == y || !mean || !invstd || !gamma || !beta || drop_p < 0.f || drop_p >= 1.f ||
        !salsa_nn_conv3x3_c64_stats_blocks(N, H, W))
        return -1;
    const unsigned nb = (unsigned)salsa_nn_conv3x3_c64_stats_blocks(N, H, W);
#if CONV_ASYNC
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    const XformArgs xf = {mean, invstd, gamma, beta, drop_args(drop_p, drop_seed)};
    hipLaunchKernelGGL((conv3x3_c64_fwd_async_kernel<false, true, true>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream,
                       (const unsigned short *)x1, (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, (const float *)nullptr,
                       (const unsigned short *)nullptr, 0, stats_part, pl.geo, xf);
#endif
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// inference: y = [relu](conv(x, w) + shift[co] [+ residual]) -- w pre-scaled by the folded BatchNorm factor gamma / sigma
extern "C" int salsa_nn_conv3x3_c64_bias_act(const void *x, const void *w, const float *shift, const void *residual, void *y,
                                             int relu, int64_t N, int H, int W, void *hip_stream)
{
    if (!x || !w || !shift || !y || x == y || N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH) return -1;
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    const unsigned nb = (unsigned)(pl.tiles >= 16384 ? CONV_BIG_GRID : pl.tiles >= 512 ? 512 : pl.tiles);
#if CONV_ASYNC && CONV_RES_EARLY
    if (residual)
        hipLaunchKernelGGL((conv3x3_c64_fwd_async_kernel<false, false, false, true>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream,
                           (const unsigned short *)x, (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, shift,
                           (const unsigned short *)residual, relu, (double *)nullptr, pl.geo);
    else
#endif
    hipLaunchKernelGGL(CONV_FWD_KERNEL<false>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned short *)x,
                       (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, shift, (const unsigned short *)residual, relu,
                       (double *)nullptr C64_GEO_ARG(pl));
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// the same with the 2x2 average pool that follows fused in: y is [N][H/2][W/2][64]; H and W must be even
extern "C" int salsa_nn_conv3x3_c64_bias_act_pool(const void *x, const void *w, const float *shift, const void *residual, void *y,
                                                  int relu, int64_t N, int H, int W, void *hip_stream)
{
    if (!x || !w || !shift || !y || x == y || N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || RPW != 2 ||
        N * H * W >= INT32_MAX / CH)
        return -1;
    const C64Plan pl = c64_plan(N, H, W, TH, TW);
    const unsigned nb = (unsigned)(pl.tiles >= 16384 ? CONV_BIG_GRID : pl.tiles >= 512 ? 512 : pl.tiles);
#if CONV_ASYNC && CONV_RES_EARLY
    if (residual)
        hipLaunchKernelGGL((conv3x3_c64_fwd_async_kernel<true, false, false, true>), dim3(nb), dim3(256), 0, (hipStream_t)hip_stream,
                           (const unsigned short *)x, (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, shift,
                           (const unsigned short *)residual, relu, (double *)nullptr, pl.geo);
    else
#endif
    hipLaunchKernelGGL(CONV_FWD_KERNEL<true>, dim3(nb), dim3(256), 0, (hipStream_t)hip_stream, (const unsigned short *)x,
                       (const unsigned short *)w, (unsigned short *)y, (int)N, pl.Hk, pl.Wk, shift, (const unsigned short *)residual, relu,
                       (double *)nullptr C64_GEO_ARG(pl));
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
