// bank_batch.h -- per-element arithmetic of the training augmentation, shared by salsa_augment_batch / salsa_augment_gcc_batch
// (feature_utils.hip: a feature batch [B][C][T][F] in, the augmented batch out) and salsa_bank_batch (bank_batch.hip: the same
// result gathered straight from the feature bank [C][bank_frames][F]).  One call = all C channels of one (clip, frame, bin): which
// cutout rectangle covers it (last rectangle wins), the fill value lo + (hi - lo) * u, the reflect-shifted source bin, the loads,
// and the swap's sign flips and differences.  The kernels differ only in where a sample's (channel 0, frame 0) lies and how far
// apart its channels are, so their results are equal bit for bit by construction.  Host + device inline functions: the same header
// compiles with g++ (tests/hostemu/bank_batch_emu.cpp), so the arithmetic is checked against the torch operators on the CPU.
// That host build is a test harness, never a fallback of the product.
//
// Reference semantics (paths relative to the upstream repository): utilities/transforms.py -- TfmapRandomSwapChannelFoa :365-437,
// TfmapRandomSwapChannelMic :440-523, GccRandomSwapChannelMic :526-618, RandomShiftUpDownNp :286-320, the cutouts :58-283.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BANK_HD __host__ __device__ __forceinline__
#else
#define BANK_HD inline
#endif

namespace bank_batch {

// par: int32 [NPAR] per sample = m0..m3, shift, up, 0, 0, top[8], h[8], left[8], w[8]
constexpr int NPAR = 40;
enum { RECIPE_NONE = 0, RECIPE_FOA = 1, RECIPE_MIC = 2, RECIPE_GCC = 3 };

// per case (0: none, 1: m0, 2: m1, 3: m2 -- the first set bit): output row c = input row GCC_SRC[case][c], lag-flipped where
// GCC_FLIP[case][c] (transforms.py:568-602).  Functions, not tables: one definition for the host and the device.
BANK_HD int gcc_src(int k, int c)
{
    const signed char t[4][10] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9},  // no swap
                                  {0, 2, 1, 3, 5, 4, 6, 7, 9, 8},  // m0: swap M2 / M3
                                  {3, 1, 2, 0, 8, 9, 6, 7, 4, 5},  // m1: swap M1 / M4
                                  {1, 0, 3, 2, 4, 8, 7, 6, 5, 9}}; // m2: swap M1 / M2 and M3 / M4
    return t[k][c];
}
BANK_HD int gcc_flip(int k, int c)
{
    const signed char t[4][10] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                  {0, 0, 0, 0, 0, 0, 0, 1, 0, 0},
                                  {0, 0, 0, 0, 1, 1, 1, 0, 1, 1},
                                  {0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    return t[k][c];
}

// the last rectangle that covers (t, f), -1 for none
BANK_HD int hit_rect(const int *p, int t, int f)
{
    int hit = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        const int top = p[8 + r], h = p[16 + r], left = p[24 + r], w = p[32 + r];
        if (t >= top && t < top + h && f >= left && f < left + w) hit = r;
    }
    return hit;
}

// min + (max - min) * u as three rounded operations, like the torch restatement (no FMA; the g++ harness: -ffp-contract=off)
BANK_HD float fill_value(float lo, float hi, float u)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    const float d = hi - lo;
    const float m = d * u;
    return lo + m;
}

// the source bin of output bin f under a shift of s bins (np.pad(mode='reflect') semantics)
BANK_HD int shift_source(const int *p, int f, int F)
{
    const int s = p[4];
    int fs = f;
    if (s > 0) {
        if (p[5]) fs = f - s < 0 ? s - f : f - s;                    // shifted up: pad s bins at the front (reflect at bin 0)
        else fs = f + s > F - 1 ? 2 * (F - 1) - (f + s) : f + s;       // shifted down: pad at the back (reflect at bin F-1)
    }
    return fs;
}

// The channel swap of the seven FOA / MIC SALSA (and IV) rows of one (frame, bin), in place: p[0..3] the swap bits (MIC: three).  The
// MIC bits act one after the other on the running values, so several set bits give the reference's sequential float32 differences.
// augment7's swap and tta.h's variant body are this one statement.
BANK_HD void swap7(float *x, bool mic, const int *p)
{
    if (!mic) { // W Y Z X | Iy Iz Ix : swap x<->y, negate x, y, z
        if (p[0]) { float a = x[1]; x[1] = x[3]; x[3] = a; a = x[4]; x[4] = x[6]; x[6] = a; }
        if (p[1]) x[6] = -x[6];
        if (p[2]) x[4] = -x[4];
        if (p[3]) x[5] = -x[5];
    } else {    // M1 M2 M3 M4 | p12 p13 p14
        if (p[0]) { float a = x[1]; x[1] = x[2]; x[2] = a; a = x[4]; x[4] = x[5]; x[5] = a; }
        if (p[1]) {
            const float c0 = x[0], c3 = x[3], c4 = x[4], c5 = x[5], c6 = x[6];
            x[0] = c3; x[3] = c0;
            x[6] = -c6; x[5] = c5 - c6; x[4] = c4 - c6;
        }
        if (p[2]) {
            const float c0 = x[0], c1 = x[1], c2 = x[2], c3 = x[3], c4 = x[4], c5 = x[5], c6 = x[6];
            x[0] = c1; x[1] = c0; x[2] = c3; x[3] = c2;
            x[4] = -c4; x[5] = c6 - c4; x[6] = c5 - c4;
        }
    }
}

// FOA / MIC SALSA (and IV) rows: src = the sample's (channel 0, frame 0, bin 0), chan = elements between its channels; dst = the
// output element of channel 0, plane = elements between the output's channels.  minmax = the sample's (lo, hi).
BANK_HD void augment7(const float *src, int64_t chan, float *dst, int64_t plane, int t, int f, int F, bool mic, int n_zero,
                      const int *p, const float *uval, const float *minmax)
{
    const int hit = hit_rect(p, t, f);
    if (hit >= 0) {
        const float v = fill_value(minmax[0], minmax[1], uval[hit]);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < 7; c++) dst[c * plane] = c < 7 - n_zero ? v : 0.f;
        return;
    }
    const int fs = shift_source(p, f, F);
    float x[7];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 7; c++) x[c] = src[c * chan + (int64_t)t * F + fs];
    swap7(x, mic, p);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 7; c++) dst[c * plane] = x[c];
}

// The baseline GCC rows M1..M4 | xc12 xc13 xc14 xc23 xc24 xc34: pure gathers, every output is an input value or the fill value.
BANK_HD void augment10(const float *src, int64_t chan, float *dst, int64_t plane, int t, int f, int F, const int *p,
                       const float *uval, const float *minmax)
{
    const int hit = hit_rect(p, t, f);
    if (hit >= 0) {
        const float v = fill_value(minmax[0], minmax[1], uval[hit]);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < 10; c++) dst[c * plane] = c < 4 ? v : 0.f;
        return;
    }
    int fs = shift_source(p, f, F);
    fs = fs < 0 ? 0 : fs > F - 1 ? F - 1 : fs;        // (a shift of F bins or more: stay inside the row)
    const int k = p[0] ? 1 : p[1] ? 2 : p[2] ? 3 : 0;
    const float *row = src + (int64_t)t * F;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 10; c++) {
        const int g = c < 4 ? fs : f;                  // the shift moves the spectrogram rows only
        const int gf = gcc_flip(k, c) ? F - 1 - g : g; // the swap's lag flip, taken before the shift
        dst[c * plane] = row[gcc_src(k, c) * chan + gf];
    }
}

// The target half of the swaps (augment.swap_targets): element (col) of one label frame's [x | y | z] row `row` of 3 nc values.
// foa: bit 0 swaps x and y, bits 1..3 negate x, y, z.  mic (and gcc): bit 0 swaps x and y, bit 1 swaps them and negates both,
// bit 2 negates y and z.  Negation and selection only: exact.
BANK_HD float swap_target(const float *row, int col, int nc, bool foa, const int *p)
{
    const int axis = col / nc, k = col - axis * nc;
    int src = axis;                                    // which input axis lands on this output axis
    bool neg = false;
    if (foa) {
        if (p[0] && axis < 2) src = 1 - axis;
        neg = axis == 0 ? p[1] != 0 : axis == 1 ? p[2] != 0 : p[3] != 0;
    } else {
        if (p[0] && axis < 2) src = 1 - src;
        if (p[1] && axis < 2) { src = 1 - src; neg = !neg; }
        if (p[2] && axis >= 1) neg = !neg;
    }
    const float v = row[src * nc + k];
    return neg ? -v : v;
}

} // namespace bank_batch
