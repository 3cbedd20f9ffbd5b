// conv_stem.hip -- the CRNN's first convolution, 3x3 / stride 1 / pad 1, Cin <= 16 feature channels -> 64, on the gfx950 matrix
// cores: reads the extractor's planar float32 output, writes channels-last bf16 (forward; its weight gradient: conv_stem_wrw.hip).
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_internal.h"

#ifndef STEM_OUT_NT
#define STEM_OUT_NT 0
#endif

// ------------------------------------------------------------------------------------------------------------ stem layer
// The network's first convolution: Cin <= 8 feature channels (7 for SALSA) -> 64, reading the extractor's OWN output layout
// (float32, planar [N][Cin][H][W]) -- no layout change, no cast pass.  One workgroup = one 8 x 32 pixel tile: the halo tile goes
// to LDS as [pixel][8 channels] bf16 (16 B per pixel, channels Cin..7 zero), which makes a B fragment (one pixel, one tap, 8
// channels = 8 consecutive K) a single ds_read_b128.  K = 10 taps x 8 (tap 9 has zero weights) = 5 MFMA steps; the filter
// (64 x 80 bf16, prepared by the caller) sits in registers.  The layer is bound by its 64-channel output stream, so the
// optional epilogue (folded BatchNorm shift + ReLU, inference) saves a whole read + write of that tensor.
namespace {

#ifdef STEM_NO_STORE // probe: every value computed, nothing written
#define STEM_STORE_COND &&v.x == 0x12345678u && v.w == 0x9abcdef0u
#else
#define STEM_STORE_COND
#endif
constexpr int STH = 8, SHALO_H = STH + 2; // stem tile: 8 rows x TW pixels, wave w owns rows 2w, 2w+1 and all 64 output channels

// STATS (training): the launch is persistent (a workgroup walks tiles blockIdx.x, + gridDim.x, ...) and also leaves the
// per-channel sum / sum of squares of its bf16-rounded outputs as one float64 row [2][64] per workgroup for the BatchNorm that
// follows, accumulated like the 64 -> 64 kernel's (conv64_stats: DPP quad sums, lane q of a quad keeps channel group q).
#ifndef STEM_FWD_WPS
#define STEM_FWD_WPS 2 // round 5: with (256, 1) the compiler parked the accumulators in 64 AGPRs next to 160 - 208 VGPRs: one (training) / two (inference) waves per SIMD; held to 256 / 2 registers they stay in VGPRs: two / three waves, 277 -> 210 us (training, with the statistics epilogue), 0.361 -> 0.313 ms (inference sub-batch)
#endif
// NG = 2 (9 <= Cin <= 16, the baseline GCC features' 10 channels): a halo pixel holds 16 bf16 channels (32 B), one K step is one
// tap across all 16 (lanes 0-31 channels 0-7, lanes 32-63 channels 8-15): 9 steps, no padding tap; filter [64][9 taps][16].
template <bool STATS, int NG = 1>
__global__ __launch_bounds__(256, STEM_FWD_WPS) void conv3x3_stem_fwd_kernel(const float *__restrict__ x, const unsigned short *__restrict__ wq,
                                                               unsigned short *__restrict__ y, int N, int Cin, int H, int W, long x_batch_stride,
                                                               long x_channel_stride, const float *__restrict__ shift, int relu,
                                                               double *__restrict__ stats_part)
{
    constexpr int PCH = 8 * NG, KSTEPS = NG == 1 ? 5 : 9; // channels per halo pixel, K steps
    __shared__ __attribute__((aligned(16))) unsigned short xs2[2][SHALO_H * HALO_W * PCH]; // double-buffered halo tile (round 4)
    __shared__ __attribute__((aligned(16))) unsigned short ys[4 * TW * ROW]; // per wave: one output row, [pixel][ROW]
    __shared__ __attribute__((aligned(16))) float shs[64]; // the folded-BatchNorm shift (inference), read from LDS in the epilogue: as
                                                           // global loads inside the tile loop they were 16 DEPENDENT round trips per
                                                           // tile (`global_load_dwordx4; s_waitcnt vmcnt(0)` per channel group and row)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int px = lane & 31, khalf = lane >> 5;
    if (tid < 64) shs[tid] = shift ? shift[tid] : 0.f; // (the first barrier of the tile loop publishes it)
    bf16x8 af[KSTEPS][2]; // [K step][co half]: filter row co = 32*mt + (lane&31), tap 2*step + khalf, its 8 channels (NG = 2: tap step, channels 8*khalf..)
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++)
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
            af[ks][mt] = NG == 1 ? *(const bf16x8 *)(wq + ((mt * 32 + px) * 10 + 2 * ks + khalf) * 8)
                                 : *(const bf16x8 *)(wq + ((mt * 32 + px) * 9 + ks) * 16 + 8 * khalf);
    const int tiles_w = (W + TW - 1) / TW, tiles_h = (H + STH - 1) / STH;
    const long n_tiles = (long)N * tiles_h * tiles_w;
    float rs[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, rq[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // Round 4.  Counters on the round-3 kernel (tools/probes/pmc_probe.sh): waves spent 65 % of their cycles waiting with the
    // VALU 25 % and the matrix pipe 8 % busy, at ~2 resident waves per SIMD.  What they waited for: __syncthreads() is a fence + a
    // barrier, i.e. `s_waitcnt vmcnt(0)` -- twice per tile every wave sat out the acknowledgement of the 32 KB it had just
    // STORED (and, at the top of a tile, the whole latency of the halo loads it had just issued).  Now: the launch is persistent
    // in both variants; the halo tile is double-buffered in LDS; the barriers are raw `s_barrier`s behind `s_waitcnt lgkmcnt(0)`
    // (LDS visibility is all they have to order); and a tile's global loads are issued TWO tiles ahead and converted into the
    // other LDS buffer between the MFMAs and the epilogue of the tile before -- the one place where everything older in the
    // memory queue (the loads themselves, one tile old, and the stores of the tile before that) has long retired, so the
    // compiler's vmcnt(0) in front of the conversion costs nothing and no wait ever follows a store.
    constexpr int SPF = (SHALO_H * HALO_W + 255) / 256; // halo pixels per thread
    float pv[SPF][PCH];
    bool pin[SPF];
    // Round 5 (as in the weight gradient below, where the same three changes took 14 % off an issue-bound kernel): tile coordinates
    // from cursors stepped by the grid size with carries instead of 64-bit divisions (two decodes per tile), every address = a
    // wave-uniform 64-bit base + a 32-bit offset, validity by unsigned compares joined with `&` (no nested EXEC-mask regions)
    struct Cursor { int tw, th, n; };
    const int G_ = (int)gridDim.x;
    const int dgw = G_ % tiles_w, dgh = (G_ / tiles_w) % tiles_h, dgn = G_ / (tiles_w * tiles_h);
    auto cursor_at = [&](long t) {
        Cursor c;
        c.tw = (int)(t % tiles_w); c.th = (int)((t / tiles_w) % tiles_h); c.n = (int)(t / ((long)tiles_w * tiles_h));
        return c;
    };
    auto advance = [&](Cursor &c) {
        c.tw += dgw;
        if (c.tw >= tiles_w) { c.tw -= tiles_w; c.th += 1; }
        c.th += dgh;
        if (c.th >= tiles_h) { c.th -= tiles_h; c.n += 1; }
        c.n += dgn;
    };
    const int xcs32 = (int)x_channel_stride;
    auto prefetch = [&](const Cursor &t) {
        const int tw = t.tw, th = t.th;
        const float *xn = x + (long)t.n * x_batch_stride;
#pragma unroll
        for (int j = 0; j < SPF; j++) { // neighbouring lanes = neighbouring columns: every plane's loads coalesce
            const int p = tid + j * 256;
            const int hh = p / HALO_W, ww = p - hh * HALO_W;
            const int h = th * STH + hh - 1, wcol = tw * TW + ww - 1;
            pin[j] = (p < SHALO_H * HALO_W) & ((unsigned)h < (unsigned)H) & ((unsigned)wcol < (unsigned)W);
            const unsigned o = pin[j] ? (unsigned)(h * W + wcol) : 0u;
#pragma unroll
            for (int c = 0; c < PCH; c++) { // unconditional (valid) loads.  NOT `c < Cin ? c * stride : 0`: the compiler then re-used the
                const int cc = c < Cin ? c : Cin - 1; // c = 0 load for the planes beyond Cin behind a `s_waitcnt vmcnt(0)` -- a full
                pv[j][c] = xn[o + (unsigned)(cc * xcs32)]; // memory round trip in the middle of every prefetch
            }
        }
    };
    auto convert = [&](int buf) { // registers -> bf16 [pixel][PCH channels] in LDS: one 16-byte write per 8 channels of a pixel
#pragma unroll
        for (int j = 0; j < SPF; j++) {
            const int p = tid + j * 256;
            if constexpr (NG == 1) {
                uint4 pk;
                pk.x = pack_bf16((pin[j] && 0 < Cin) ? pv[j][0] : 0.f, (pin[j] && 1 < Cin) ? pv[j][1] : 0.f);
                pk.y = pack_bf16((pin[j] && 2 < Cin) ? pv[j][2] : 0.f, (pin[j] && 3 < Cin) ? pv[j][3] : 0.f);
                pk.z = pack_bf16((pin[j] && 4 < Cin) ? pv[j][4] : 0.f, (pin[j] && 5 < Cin) ? pv[j][5] : 0.f);
                pk.w = pack_bf16((pin[j] && 6 < Cin) ? pv[j][6] : 0.f, (pin[j] && 7 < Cin) ? pv[j][7] : 0.f);
                if (p < SHALO_H * HALO_W) *(uint4 *)(xs2[buf] + p * 8) = pk;
            } else {
                uint4 pk[NG];
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    const int c0 = 8 * g;
                    pk[g].x = pack_bf16((pin[j] && c0 + 0 < Cin) ? pv[j][c0 + 0] : 0.f, (pin[j] && c0 + 1 < Cin) ? pv[j][c0 + 1] : 0.f);
                    pk[g].y = pack_bf16((pin[j] && c0 + 2 < Cin) ? pv[j][c0 + 2] : 0.f, (pin[j] && c0 + 3 < Cin) ? pv[j][c0 + 3] : 0.f);
                    pk[g].z = pack_bf16((pin[j] && c0 + 4 < Cin) ? pv[j][c0 + 4] : 0.f, (pin[j] && c0 + 5 < Cin) ? pv[j][c0 + 5] : 0.f);
                    pk[g].w = pack_bf16((pin[j] && c0 + 6 < Cin) ? pv[j][c0 + 6] : 0.f, (pin[j] && c0 + 7 < Cin) ? pv[j][c0 + 7] : 0.f);
                }
                if (p < SHALO_H * HALO_W) {
#pragma unroll
                    for (int g = 0; g < NG; g++) *(uint4 *)(xs2[buf] + p * PCH + 8 * g) = pk[g];
                }
            }
        }
    };
#define STEM_BARRIER()                                       \
    do {                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   \
        __builtin_amdgcn_s_barrier();                        \
    } while (0)
    Cursor cur = cursor_at(blockIdx.x), pf = cur; // this tile / the next tile to request
    if ((long)blockIdx.x < n_tiles) {
        prefetch(pf);
        advance(pf);
        convert(0);
        if ((long)blockIdx.x + gridDim.x < n_tiles) {
            prefetch(pf);
            advance(pf);
        }
    }
    int it = 0;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, it++, advance(cur)) {
    STEM_BARRIER(); // tile's LDS copy is complete (every wave's part), and the other buffer's readers (the tile before) are done
    const unsigned short *xs = xs2[it & 1];
    const int tw = cur.tw, th = cur.th;
    unsigned short *yb = y + (long)cur.n * H * W * CH; // this image (wave-uniform); the stores add 32-bit offsets
    f32x16 acc[2][2];
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
        for (int mt = 0; mt < 2; mt++) acc[rr][mt] = f32x16{};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) {
        const int tap = NG == 2 ? ks : 2 * ks + khalf < 9 ? 2 * ks + khalf : 8; // tap 9: any address, its weights are zero
        const int r = tap / 3, sx = tap - 3 * r;
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const bf16x8 b = *(const bf16x8 *)(xs + ((wv * 2 + rr + r) * HALO_W + px + sx) * PCH + (NG == 2 ? 8 * khalf : 0));
#pragma unroll
            for (int mt = 0; mt < 2; mt++) acc[rr][mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks][mt], b, acc[rr][mt], 0, 0, 0);
        }
    }
    if (tile + gridDim.x < n_tiles) { // the next tile: its loads are one tile old -> the other LDS buffer; then the loads of the tile after
        convert((it + 1) & 1);
        if (tile + 2 * (long)gridDim.x < n_tiles) {
            prefetch(pf);
            advance(pf);
        }
    }
    // Epilogue.  D gives a lane four groups of four consecutive output channels of ONE pixel: stored directly that is 8-byte
    // pieces, 16 store instructions per 128-byte pixel.  Each wave turns its row around through a private LDS strip
    // ([pixel][64 co], rows padded to 144 bytes) instead and writes 16 bytes per lane, 8 lanes per pixel: every store
    // instruction covers 8 whole pixels = 1 KB of contiguous memory (0.62 -> 0.52 ms on an 8 x 4800 x 200 sub-batch).
    unsigned short *strip = ys + wv * (TW * ROW);
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int g = 0; g < 4; g++) { // D rows (reg&3) + 8*(reg>>2) + 4*(lane>>5): four consecutive output channels
                float v4[4] = {acc[rr][mt][4 * g], acc[rr][mt][4 * g + 1], acc[rr][mt][4 * g + 2], acc[rr][mt][4 * g + 3]};
                if (shift) {
                    const float4 sh = *(const float4 *)(shs + 32 * mt + 4 * khalf + 8 * g);
                    v4[0] += sh.x; v4[1] += sh.y; v4[2] += sh.z; v4[3] += sh.w;
                    if (relu) {
#pragma unroll
                        for (int j = 0; j < 4; j++) v4[j] = fmaxf(v4[j], 0.f);
                    }
                }
                uint2 v;
                v.x = pack_bf16(v4[0], v4[1]);
                v.y = pack_bf16(v4[2], v4[3]);
                *(uint2 *)(strip + px * ROW + 32 * mt + 8 * g + 4 * khalf) = v;
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the strip is wave-private: no barrier, only LDS order
        const int h = th * STH + wv * 2 + rr;
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int p = it * 8 + (lane >> 3), piece = lane & 7;
            const uint4 v = *(const uint4 *)(strip + p * ROW + piece * 8);
            const int wcol = tw * TW + p;
            if ((h < H) & (wcol < W) STEM_STORE_COND) {
#if STEM_OUT_NT // round-5 probe: the first layer's output stores non-temporal
                typedef unsigned u4v_t __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(u4v_t{v.x, v.y, v.z, v.w}, (u4v_t *)(yb + (unsigned)((h * W + wcol) * CH + piece * 8)));
#else
                *(uint4 *)(yb + (unsigned)((h * W + wcol) * CH + piece * 8)) = v;
#endif
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the next row overwrites the strip
    }
    if (STATS) { // the wave's rows 8 th + 2 wv + {0, 1} = conv64_stats' rows (4 th' + 2 rg + rr) with th' = 2 th + wv / 2, rg = wv & 1
#pragma unroll
        for (int mt = 0; mt < 2; mt++) {
            const f32x16 a2[2] = {acc[0][mt], acc[1][mt]};
            conv64_stats(a2, rs[mt], rq[mt], 2 * th + (wv >> 1), tw, H, W, px, wv & 1);
        }
    }
    } // tile loop
    if (STATS) {
        float *lstats = (float *)ys; // [wave][sum | sum of squares][64]: the strips are free now
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int d = 4; d <= 16; d <<= 1) {
                    rs[mt][j] += __shfl_xor(rs[mt][j], d);
                    rq[mt][j] += __shfl_xor(rq[mt][j], d);
                }
        if (px < 4) {
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    lstats[wv * 128 + 32 * mt + 4 * khalf + 8 * px + j] = rs[mt][j];
                    lstats[wv * 128 + 64 + 32 * mt + 4 * khalf + 8 * px + j] = rq[mt][j];
                }
        }
        __syncthreads();
        if (tid < 128)
            stats_part[(long)blockIdx.x * 128 + tid] = (double)lstats[tid] + (double)lstats[128 + tid] + (double)lstats[256 + tid] + (double)lstats[384 + tid];
    }
}

} // namespace

#ifndef STEM_FWD_GRID
#define STEM_FWD_GRID 1536
#endif
#ifndef STEM_STATS_GRID
#define STEM_STATS_GRID 1024
#endif
/* number of partial rows salsa_nn_conv3x3_stem_stats writes (= its persistent workgroup count) */
extern "C" int salsa_nn_conv3x3_stem_stats_blocks(int64_t N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH) return 0;
    const long tiles = (long)N * ((H + STH - 1) / STH) * ((W + TW - 1) / TW);
    return (int)(tiles >= STEM_STATS_GRID ? STEM_STATS_GRID : tiles);
}

// training: the plain first-layer convolution from a persistent launch that also leaves its output's per-channel partial sums
// (float64 rows stats_part[blocks][2][64]) for the BatchNorm that follows -- see salsa_nn_conv3x3_c64_stats
extern "C" int salsa_nn_conv3x3_stem_stats(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *wq, void *y,
                                           double *stats_part, int64_t N, int Cin, int H, int W, void *hip_stream)
{
    if (!x || !wq || !y || !stats_part || N <= 0 || Cin <= 0 || Cin > 16 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH ||
        x_channel_stride < (int64_t)H * W || x_batch_stride < x_channel_stride * Cin ||
        x_channel_stride * Cin >= INT32_MAX /* 32-bit element offsets inside an image */)
        return -1;
    const unsigned nb = (unsigned)salsa_nn_conv3x3_stem_stats_blocks(N, H, W);
    hipLaunchKernelGGL((Cin <= 8 ? conv3x3_stem_fwd_kernel<true> : conv3x3_stem_fwd_kernel<true, 2>), dim3(nb), dim3(256), 0,
                       (hipStream_t)hip_stream, x, (const unsigned short *)wq, (unsigned short *)y, (int)N, Cin, H, W, (long)x_batch_stride,
                       (long)x_channel_stride, (const float *)nullptr, 0, stats_part);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}

// x float32 planar [N][Cin][H][W] (Cin <= 16; rows contiguous, batch / channel strides in elements, so a time-cropped view of
// the extractor's output needs no copy), wq bf16 [64][10][8] = w[co][tap][ci] zero-padded (tap 9 and ci >= Cin zero) for
// Cin <= 8, [64][9][16] = w[co][tap][ci] (ci >= Cin zero) for 9 <= Cin <= 16;
// y bf16 channels-last [N][H][W][64]; shift NULL: plain convolution, else y = [relu](conv + shift[co]) (folded BatchNorm)
extern "C" int salsa_nn_conv3x3_stem(const float *x, int64_t x_batch_stride, int64_t x_channel_stride, const void *wq,
                                     const float *shift, void *y, int relu, int64_t N, int Cin, int H, int W, void *hip_stream)
{
    if (!x || !wq || !y || N <= 0 || Cin <= 0 || Cin > 16 || H <= 0 || W <= 0 || N * H * W >= INT32_MAX / CH ||
        x_channel_stride < (int64_t)H * W || x_batch_stride < x_channel_stride * Cin ||
        x_channel_stride * Cin >= INT32_MAX /* 32-bit element offsets inside an image */)
        return -1;
    const long tiles = (long)N * ((H + STH - 1) / STH) * ((W + TW - 1) / TW);
    if (tiles >= INT32_MAX) return -1;
    const unsigned nb = (unsigned)(tiles >= STEM_FWD_GRID ? STEM_FWD_GRID : tiles); // persistent: six workgroups per CU
    hipLaunchKernelGGL((Cin <= 8 ? conv3x3_stem_fwd_kernel<false> : conv3x3_stem_fwd_kernel<false, 2>), dim3(nb), dim3(256), 0,
                       (hipStream_t)hip_stream, x, (const unsigned short *)wq, (unsigned short *)y, (int)N, Cin, H, W, (long)x_batch_stride,
                       (long)x_channel_stride, shift, relu, (double *)nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
