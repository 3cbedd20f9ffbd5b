// tta.h -- per-element arithmetic of test-time augmentation, shared by the kernels of tta.hip and the g++
// harness tests/hostemu/tta_emu.cpp (host + device inline functions, the BANK_HD pattern of bank_batch.h; that host build is a test
// harness, never a fallback of the product).
//   variant_bits      variant index v of a recipe kind -> the swap bits m the training augmentation would have drawn
//   variant7 / 10     W consecutive elements of all C channels of one sample under those bits: bank_batch::swap7 (FOA / MIC) and the
//                     bank_batch::gcc_src / gcc_flip gather (GCC) -- what augment7 / augment10 compute with no shift and no cutout
//   unswap3           the inverse of bank_batch::swap_target on one class's (x, y, z): every bit's step is a signed permutation and its
//                     own inverse, so the inverse applies the steps in REVERSE bit order; selection and negation only: exact
//   merge_one         one (clip, label frame, class) of the merge: its N = models x variants outputs un-swapped and added in float32,
//                     models outer and variants in list order, starting FROM the first output (no 0 + x: a -0 stays -0), then ONE
//                     correctly rounded division by float(N).  Additions and one division: nothing an FMA could contract.
#pragma once
#include <stdint.h>
#include "bank_batch.h"

#if defined(__HIPCC__)
#define TTA_UNROLL _Pragma("unroll")
#else
#define TTA_UNROLL
#endif

namespace tta {

enum { KIND_FOA = 1, KIND_MIC = 2, KIND_GCC = 3 }; // = bank_batch::RECIPE_* / SALSA_BANK_*
constexpr int MAX_VARIANTS = 16;                   // the largest V; also the cap on a call's variant list

struct ids_t { int v[MAX_VARIANTS]; };             // a call's variant list, handed to the kernel by value

BANK_HD int n_variants(int kind) { return kind == KIND_FOA ? 16 : kind == KIND_MIC ? 8 : kind == KIND_GCC ? 4 : 0; }

// foa / mic: m[j] = bit j of v.  gcc: v = 0 no swap, v = 1, 2, 3 the one-hot m with bit v - 1 set (GccRandomSwapChannelMic acts on
// the first set bit only, so the one-hot patterns are all there is)
BANK_HD void variant_bits(int kind, int v, int *m)
{
    TTA_UNROLL
    for (int j = 0; j < 4; j++) m[j] = kind == KIND_GCC ? (v == j + 1 && j < 3) : ((v >> j) & 1);
    if (kind != KIND_FOA) m[3] = 0;
}

template <int W> struct pack;
template <> struct pack<1> { float v[1]; };
template <> struct pack<4> { alignas(16) float v[4]; };

// elements e .. e + W - 1 of the sample's (T, F) plane, all seven channels.  src: the sample's channel 0, chan: elements between its
// channels; dst: the output sample's channel 0, plane: elements between the output's channels (= T F).  W = 4: e, chan, plane and both
// pointers are multiples of four elements / 16 bytes (the launcher checks), so every access is one 16-byte access.
template <int W> BANK_HD void variant7(const float *src, int64_t chan, float *dst, int64_t plane, int64_t e, bool mic, const int *m)
{
    pack<W> in[7], out[7];
    TTA_UNROLL
    for (int c = 0; c < 7; c++) in[c] = *(const pack<W> *)(src + c * chan + e);
    TTA_UNROLL
    for (int j = 0; j < W; j++) {
        float x[7];
        TTA_UNROLL
        for (int c = 0; c < 7; c++) x[c] = in[c].v[j];
        bank_batch::swap7(x, mic, m);
        TTA_UNROLL
        for (int c = 0; c < 7; c++) out[c].v[j] = x[c];
    }
    TTA_UNROLL
    for (int c = 0; c < 7; c++) *(pack<W> *)(dst + c * plane + e) = out[c];
}

// the same for the ten GCC rows: bins f .. f + W - 1 of frame t (W = 4: F a multiple of four as well, so the lag-flipped source
// F - W - f .. F - 1 - f is one aligned 16-byte access read back to front).  k = the swap case (0 none, 1..3 the set bit + 1).
template <int W> BANK_HD void variant10(const float *src, int64_t chan, float *dst, int64_t plane, int t, int f, int F, int k)
{
    const int64_t row = (int64_t)t * F;
    TTA_UNROLL
    for (int c = 0; c < 10; c++) {
        const float *s = src + bank_batch::gcc_src(k, c) * chan + row;
        pack<W> a;
        if (bank_batch::gcc_flip(k, c)) {
            const pack<W> r = *(const pack<W> *)(s + (F - W - f));
            TTA_UNROLL
            for (int j = 0; j < W; j++) a.v[j] = r.v[W - 1 - j];
        } else {
            a = *(const pack<W> *)(s + f);
        }
        *(pack<W> *)(dst + c * plane + row + f) = a;
    }
}

// S_m^-1 on one class's direction.  foa: S = (bit 0: swap x, y) then (bits 1..3: negate x, y, z).  mic and gcc: S = (bit 0: swap x, y)
// then (bit 1: swap x, y and negate both) then (bit 2: negate y, z).
BANK_HD void unswap3(float &x, float &y, float &z, bool foa, const int *m)
{
    float a = x, b = y, c = z;                         // (selects on by-value copies: the values stay in registers)
    if (foa) {
        a = m[1] ? -a : a;
        b = m[2] ? -b : b;
        c = m[3] ? -c : c;
    } else {
        b = m[2] ? -b : b;
        c = m[2] ? -c : c;
        const float a1 = m[1] ? -b : a, b1 = m[1] ? -a : b;
        a = a1;
        b = b1;
    }
    x = m[0] ? b : a;
    y = m[0] ? a : b;
    z = c;
}

// prob: slab [N][cells][nc], xyz: slab [N][cells][3 nc] (blocks x | y | z); cell = clip * L + label frame, k = class.
// out4 = merged (p, x, y, z).
BANK_HD void merge_one(const float *prob, const float *xyz, int n_models, const ids_t &ids, int n_var, int kind, int64_t cells, int nc,
                       int64_t cell, int k, float *out4)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    for (int mi = 0; mi < n_models; mi++)
        for (int vi = 0; vi < n_var; vi++, n++) {
            int m[4];
            variant_bits(kind, ids.v[vi], m);
            const int64_t at = (int64_t)n * cells + cell;
            const float *d = xyz + at * 3 * nc + k;
            float x = d[0], y = d[nc], z = d[2 * nc];
            unswap3(x, y, z, kind == KIND_FOA, m);
            const float p = prob[at * nc + k];
            if (n == 0) { acc[0] = p; acc[1] = x; acc[2] = y; acc[3] = z; }
            else { acc[0] = acc[0] + p; acc[1] = acc[1] + x; acc[2] = acc[2] + y; acc[3] = acc[3] + z; }
        }
    const float fn = (float)n;
    TTA_UNROLL
    for (int j = 0; j < 4; j++) {
#if defined(__HIP_DEVICE_COMPILE__)
        out4[j] = __fdiv_rn(acc[j], fn);
#else
        out4[j] = acc[j] / fn;
#endif
    }
}

} // namespace tta
