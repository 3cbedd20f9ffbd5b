// conv_internal.h -- internal: what more than one of the 64-channel convolution units (conv_mfma.hip, conv_stem.hip,
// conv_c64_wrw.hip, conv_stem_wrw.hip) uses, and the MFMA operand types that conv_wide.hip and conv_1x1.hip share with them.
// Kernel-side names sit in an anonymous namespace, as they did inside the units: every unit gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nn_common.h" // DropArgs (XformArgs below), pack_bf16

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CH = 64;            // channels in = out
constexpr int ROW = 72;           // padded channel stride in LDS (bf16 elements): 144 bytes
#ifndef CONV_RPW
#define CONV_RPW 2 // measured: 2 rows per wave at 2 waves per SIMD (0.44 ms for 32x640x200) beats 4 rows at 1 wave per SIMD (0.50)
#endif
constexpr int RPW = CONV_RPW;      // output rows per wave
constexpr int TH = 2 * RPW, TW = 32; // output tile of a workgroup: waves = 2 row groups x 2 halves of the 64 output channels
constexpr int HALO_W = TW + 2, HALO_H = TH + 2;

// Addressing of a map in KERNEL coordinates: pixel (n, h, w) lives at element n * sn + h * sh + w * sw.  Normal: sh = W * 64, sw = 64.
// TRANSPOSED (tap_t = 1): the kernel is handed the map with its axes swapped (its H = the image's width, its W = the image's
// height, sh = 64, sw = image width * 64) and the filter taps swapped to match (conv(x)^T = conv_{w^T}(x^T)) -- nothing moves in
// memory.  Why: a tile is 4 rows x 32 columns of kernel pixels (the MFMA's 32 columns), so a 100-column map wastes 28 of every
// 128 columns and a 200-column one 24 of 224, while the CRNN's heights (640, 320, 4800, 2400) are multiples of 32 and its
// widths of 4: transposed, every tile is full (320 x 100: 250 tiles per image instead of 320).  A pixel's 64 channels are one
// contiguous 128-byte line either way.  psn / psh / psw: the same for the 2x2-pooled output of the POOL epilogue.
struct Geo {
    long sn;
    int sh, sw, tap_t;
    long psn;
    int psh, psw;
};
__device__ __forceinline__ long geo_off(const Geo &g, long n, int h, int w) { return n * g.sn + (long)h * g.sh + (long)w * g.sw; }

// Training: per-channel sum and sum of squares of the tile's bf16-ROUNDED outputs (what the BatchNorm that follows would read
// back from HBM in its own statistics pass).  A lane holds 16 channels x 2 rows of ONE pixel column.  No LDS in the tile loop
// -- LDS float atomics, even pre-reduced to 4-way conflicts, DOUBLED the kernel (0.45 -> 0.96 ms at 32 x 640 x 200) -- and no
// 32 running sums per lane either (the filter owns the register file): two DPP swaps sum each quad of neighbouring pixel
// columns, after which all four lanes of the quad hold the same 16 totals, and lane q of the quad keeps the running sums of
// channel group q only: 8 registers.  The quads are combined once, after the last tile.
__device__ __forceinline__ float dpp_xor1(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1 /* quad_perm [1,0,3,2] */, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_xor2(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E /* quad_perm [2,3,0,1] */, 0xf, 0xf, true));
}
#ifndef CONV_STATS_DOT2
#define CONV_STATS_DOT2 0 // round 5 experiment: the two rows of a channel as ONE bf16 pair, sum and sum of squares by v_dot2_f32_bf16: 144 instead of 240 vector
                          // instructions per tile-wave and NO faster (with statistics 0.442 / 0.446 -> 0.459 / 0.460 ms at 32 x 640 x 200; 36 B of scratch); off
#endif
__device__ __forceinline__ void conv64_stats(const f32x16 (&acc)[RPW], float (&rs)[4], float (&rq)[4], int th, int tw, int H, int W,
                                             int px, int rg)
{
    const int h0 = th * TH + rg * RPW, wcol = tw * TW + px;
    const int quad = px & 3;
#if CONV_STATS_DOT2 && CONV_RPW == 2
    // Round 5.  The epilogue cost what a separate statistics pass would (tools/probes/conv64_stats_probe.py: +60 - 80 us on the 311-us
    // kernel at 32 x 640 x 200): 9 vector instructions per bf16 PAIR of neighbouring channels (pack, two unpacks, two masks, two
    // adds, two FMAs) + the quad sums.  A lane's two output ROWS of one channel make a pair as well: packed once (the same
    // round-to-nearest-even as the store's), `v_dot2_f32_bf16 pair, (1, 1)` is the channel's sum over both rows and
    // `v_dot2_f32_bf16 pair, pair` its sum of squares -- 3 instructions per channel where there were 9, and the row mask of an edge tile
    // is one AND on the pair (skipped, wave-uniformly, on interior tiles).
    const bool row1 = h0 + 1 < H;                                    // wave-uniform
    const unsigned keep_rows = !(h0 < H) ? 0u : row1 ? 0xffffffffu : 0x0000ffffu;
    const unsigned lane_mask = wcol < W ? keep_rows : 0u;            // per lane: the pixel column may lie outside the map
    const bool edge = !row1 || tw * TW + TW > W;                     // wave-uniform: some lane or row of this wave's tile part is outside
    const unsigned ones = 0x3f803f80u;                               // bf16 (1, 1)
#pragma unroll
    for (int g = 0; g < 4; g++) {
        float t[4], q[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned pr = pack_bf16(acc[0][4 * g + j], acc[1][4 * g + j]);
            if (edge) pr &= lane_mask;
            asm("v_dot2_f32_bf16 %0, %1, %2, 0" : "=v"(t[j]) : "v"(pr), "v"(ones));
            asm("v_dot2_f32_bf16 %0, %1, %1, 0" : "=v"(q[j]) : "v"(pr));
        }
        const float keep = quad == g ? 1.f : 0.f; // lane `quad` of each quad keeps channel group g = quad
#pragma unroll
        for (int j = 0; j < 4; j++) {
            t[j] += dpp_xor1(t[j]); q[j] += dpp_xor1(q[j]);
            t[j] += dpp_xor2(t[j]); q[j] += dpp_xor2(q[j]);
            rs[j] = fmaf(keep, t[j], rs[j]);
            rq[j] = fmaf(keep, q[j], rq[j]);
        }
    }
#else
    float m[RPW];
#pragma unroll
    for (int rr = 0; rr < RPW; rr++) m[rr] = (h0 + rr < H && wcol < W) ? 1.f : 0.f;
#pragma unroll
    for (int g = 0; g < 4; g++) { // accumulator elements 4 g .. 4 g + 3 = channels 8 g + j (+ the lane's base); 8 temporaries live
        float t[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 2; k++)
#pragma unroll
            for (int rr = 0; rr < RPW; rr++) {
                const unsigned u = pack_bf16(acc[rr][4 * g + 2 * k], acc[rr][4 * g + 2 * k + 1]);
                const float r0 = __uint_as_float(u << 16), r1 = __uint_as_float(u & 0xffff0000u);
                const float a0 = r0 * m[rr], a1 = r1 * m[rr];
                t[2 * k] += a0; t[2 * k + 1] += a1;
                q[2 * k] = fmaf(a0, r0, q[2 * k]); q[2 * k + 1] = fmaf(a1, r1, q[2 * k + 1]);
            }
        const float keep = quad == g ? 1.f : 0.f; // lane `quad` of each quad keeps channel group g = quad
#pragma unroll
        for (int j = 0; j < 4; j++) {
            t[j] += dpp_xor1(t[j]); q[j] += dpp_xor1(q[j]);
            t[j] += dpp_xor2(t[j]); q[j] += dpp_xor2(q[j]);
            rs[j] = fmaf(keep, t[j], rs[j]);
            rq[j] = fmaf(keep, q[j], rq[j]);
        }
    }
#endif
}

// ---- XCD-aware walk of a persistent workgroup over the (image, tile row, tile column) space (round 3).
// Workgroup b runs on XCD b % 8, each XCD with its own L2.  Dealing the tiles round-robin (tile = b + i * grid) puts vertically
// neighbouring tiles -- which share two of a tile's six halo rows -- on different XCDs, so every halo row came from HBM twice:
// rocprofv3 FETCH_SIZE of the forward kernel at 8 x 2400 x 100 was 392 MB for a 246-MB input (1.59x = the 6/4 x 34/32 halo), of
// the weight-gradient kernel 1.34 GB for 1.05 GB.  Here the flattened (image, tile row) axis is cut into bands of TW_BAND rows,
// band k belongs to XCD k % 8, and the G = grid / 8 workgroups of an XCD walk ITS bands' tiles in order: at any moment an XCD works
// on ~G consecutive tiles of a few neighbouring rows, and the shared halo rows are L2 hits.  nx = 1 (grids that are not a
// multiple of 8) degenerates to the plain round-robin order.
constexpr int TW_BAND = 4;
struct TileWalk {
    int tiles_w, tiles_h, nx, xcd, G, n_local, d_tw, d_lr;
};
struct TilePos {
    int tw, lr; // tile column, row index among this XCD's rows
};
__device__ __forceinline__ TileWalk tile_walk(int N, int tiles_h, int tiles_w, int grid, int b)
{
    TileWalk w;
    w.tiles_w = tiles_w;
    w.tiles_h = tiles_h;
    w.nx = (grid % 8 == 0 && grid >= 64) ? 8 : 1;
    w.xcd = b % w.nx;
    w.G = grid / w.nx;
    const int rows = N * tiles_h, full = rows / TW_BAND, rem = rows % TW_BAND;
    const int mine = full / w.nx + (w.xcd < full % w.nx ? 1 : 0);
    w.n_local = (mine * TW_BAND + (full % w.nx == w.xcd ? rem : 0)) * tiles_w;
    w.d_tw = w.G % tiles_w;
    w.d_lr = w.G / tiles_w;
    return w;
}
__device__ __forceinline__ TilePos tile_pos(const TileWalk &w, int s) { return {s % w.tiles_w, s / w.tiles_w}; }
__device__ __forceinline__ void tile_advance(const TileWalk &w, TilePos &p) // s += G
{
    p.tw += w.d_tw;
    const int carry = p.tw >= w.tiles_w ? 1 : 0;
    p.tw -= carry ? w.tiles_w : 0;
    p.lr += w.d_lr + carry;
}
__device__ __forceinline__ void tile_coords(const TileWalk &w, const TilePos &p, int &n, int &th)
{
    const int r = ((p.lr / TW_BAND) * w.nx + w.xcd) * TW_BAND + p.lr % TW_BAND; // global (image, tile row) index
    n = r / w.tiles_h;
    th = r - n * w.tiles_h;
}

// XF (round 4): the input is the RAW output of the convolution before (x1) and this kernel's real operand is
// a = dropout(relu(batch_norm(x1))) -- the normalised activation is never written to HBM nor read back (524 MB each way for the
// stem's first BatchNorm).  The tiles still arrive by LDS-direct loads; once a thread's own pieces of tile i+1 have landed (the
// counted wait that already exists) it rewrites them in place -- a = relu(x * scale[c] + shift[c]), the dropout mask regenerated
// from the element index exactly as bn_apply_kernel draws it (nn_common.h) -- and the barrier that opens tile i+1 publishes them.
// A thread's pieces always hold the same eight channels, so its 16 coefficients come from a 512-byte LDS table once per tile;
// halo pieces outside the image stay the zeros they were loaded as (the convolution pads the ACTIVATION with zeros).
struct XformArgs {
    const float *mean, *invstd, *gamma, *beta; // the BatchNorm's batch statistics and affine parameters, float32 [64]
    DropArgs drop;
};

// ---- the weight gradients' pixel tile and transposing LDS reads (the lane mapping: conv_c64_wrw.hip)
constexpr int WT_H = 4, WT_W = 32;                       // pixel tile
constexpr int WHALO_W = WT_W + 2, WHALO_H = WT_H + 2;

// one operand fragment = two transposing reads (pixel rows +0..3 and +4..7); issued without waiting: LDS_TR_WAIT below
struct tr_frag {
    unsigned long long lo, hi;
};
#define LDS_TR_ISSUE(f, addr, imm)                                                                                         \
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"                              \
                 : "=&v"((f).lo), "=&v"((f).hi)                                                                            \
                 : "v"(addr), "n"(imm), "n"((imm) + 4 * ROW * 2))
#define LDS_TR_WAIT(f) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"((f).lo), "+v"((f).hi))
__device__ __forceinline__ bf16x8 tr_value(const tr_frag &f)
{
    union { unsigned long long q[2]; bf16x8 v; } u;
    u.q[0] = f.lo;
    u.q[1] = f.hi;
    return u.v;
}
// waits until all but the `n` newest LDS reads have returned (they return in order), naming fragment f as now valid
#define LDS_TR_WAIT_N(f, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"((f).lo), "+v"((f).hi))

} // namespace

#ifndef CONV_ASYNC
#define CONV_ASYNC 1
#endif
#ifndef C64_TRANSPOSE
#define C64_TRANSPOSE 1 // hand the 64 -> 64 kernels the map with its axes swapped when that needs >= 5 % fewer tiles (see struct Geo)
#endif
namespace {
struct C64Plan {
    int Hk, Wk; // the map's extent in kernel coordinates
    long tiles;
    Geo geo;
};
C64Plan c64_plan(int64_t N, int H, int W, int th, int tw)
{
    const long tn = (long)N * ((H + th - 1) / th) * ((W + tw - 1) / tw), tt = (long)N * ((W + th - 1) / th) * ((H + tw - 1) / tw);
    const bool tr = C64_TRANSPOSE && CONV_ASYNC && tt * 100 < tn * 95;
    C64Plan p;
    p.Hk = tr ? W : H;
    p.Wk = tr ? H : W;
    p.tiles = tr ? tt : tn;
    p.geo.sn = (long)H * W * CH;
    p.geo.sh = tr ? CH : W * CH;
    p.geo.sw = tr ? W * CH : CH;
    p.geo.tap_t = tr ? 1 : 0;
    p.geo.psn = (long)(H / 2) * (W / 2) * CH;
    p.geo.psh = tr ? CH : (W / 2) * CH;
    p.geo.psw = tr ? (W / 2) * CH : CH;
    return p;
}
} // namespace
