// multi_accdoa.h -- per-item arithmetic of the Multi-ACCDOA output format: the ADPIT loss of one (row, class)
// item (salsa_nn_adpit_loss) and the track unification of one (frame, class) cell (salsa_nn_seld_decode_multi), both in
// multi_accdoa.hip.  Host + device inline functions with no memory traffic; the same header compiles with g++
// (tests/hostemu/multi_accdoa_emu.cpp), so every decision is checked against numpy on the CPU.  That host build is a test harness,
// never a fallback of the product.
//
// The reference has no Multi-ACCDOA; the definition is this project's (Shimada et al., ICASSP 2022, restated so that every
// decision is reproducible bit for bit): C real classes, three tracks (prediction) / slots (label) per class, pseudo-class
// p = n * C + c in the [x | y | z] layout of every other layer.
#pragma once
#include <math.h>
#include <stdint.h>
#include "seld_decode.h"

#if defined(__HIPCC__)
#define MACCDOA_HD __host__ __device__ __forceinline__
#else
#define MACCDOA_HD inline
#endif

#if defined(__HIPCC__) // (the g++ harness is built with -ffp-contract=off)
#pragma clang fp contract(off)
#endif

namespace multi_accdoa {

constexpr int N_TRACKS = 3;

// the number of candidate assignments (track 0, 1, 2 -> source) with k active slots
MACCDOA_HD int n_candidates(int k) { return k >= 2 ? 6 : 1; }

// the source that candidate `cand` gives track n; -1: the zero target (k = 0).  k = 1: 000.  k = 2: 001 010 011 100 101 110 (the
// binary digits of cand + 1: every map onto both sources).  k = 3: 012 021 102 120 201 210 (the permutations in dictionary order).
MACCDOA_HD int source_of(int k, int cand, int n)
{
    if (k == 0) return -1;
    if (k == 1) return 0;
    if (k == 2) return ((cand + 1) >> (2 - n)) & 1;
    const int first = cand >> 1, r0 = first == 0 ? 1 : 0, r1 = first == 2 ? 1 : 2;
    if (n == 0) return first;
    return ((cand & 1) != 0) == (n == 1) ? r1 : r0;
}

// One item.  P[n * 3 + a]: prediction of track n, axis a; sed[m]: the label's slot activities; T[m * 3 + a]: the slot targets.
// The active slots are compacted in slot order into k sources; the chosen candidate is the lowest index of the least cost
// e = sum over tracks (outer) and axes (inner) of (P - T)^2, one running float64 sum without fma -- a later candidate replaces the
// current one only when its cost is strictly smaller, so a NaN cost never displaces an earlier candidate.  *item_loss = e_min / 9;
// g[n * 3 + a] = (float)(2 (P - T_chosen) / denom), denom = 9 rows C as a double.  Returns the candidate index.
MACCDOA_HD int adpit_item(const float *P, const float *sed, const float *T, double denom, double *item_loss, float *g)
{
    int src[N_TRACKS], k = 0;
    for (int m = 0; m < N_TRACKS; m++)
        if (sed[m] > 0.5f) src[k++] = m;
    int chosen = 0;
    double best = 0.0;
    const int nc = n_candidates(k);
    for (int cand = 0; cand < nc; cand++) {
        double e = 0.0;
        for (int n = 0; n < N_TRACKS; n++) {
            const int s = source_of(k, cand, n);
            for (int a = 0; a < 3; a++) {
                const double d = (double)P[n * 3 + a] - (s < 0 ? 0.0 : (double)T[src[s] * 3 + a]);
                e = e + d * d;
            }
        }
        if (cand == 0 || e < best) {
            best = e;
            chosen = cand;
        }
    }
    *item_loss = best / 9.0;
    for (int n = 0; n < N_TRACKS; n++) {
        const int s = source_of(k, chosen, n);
        for (int a = 0; a < 3; a++) {
            const double d = (double)P[n * 3 + a] - (s < 0 ? 0.0 : (double)T[src[s] * 3 + a]);
            g[n * 3 + a] = (float)((2.0 * d) / denom);
        }
    }
    return chosen;
}

// similar(i, j): both active and dot > cos_unify sqrt(ni nj), float64 from the float32 inputs; no transcendental
MACCDOA_HD bool similar(bool ai, bool aj, const float *vi, const float *vj, double cos_unify)
{
    if (!(ai && aj)) return false;
    const double xi = vi[0], yi = vi[1], zi = vi[2], xj = vj[0], yj = vj[1], zj = vj[2];
    const double dot = (xi * xj + yi * yj) + zi * zj;
    const double ni = (xi * xi + yi * yi) + zi * zi, nj = (xj * xj + yj * yj) + zj * zj;
    return dot > cos_unify * sqrt(ni * nj);
}

// One (frame, class) cell.  act[n]: track activities, v[n * 3 + a]: track vectors.  out[g * 3 + a]: the emitted vectors in group
// order (groups ordered by their lowest track); flags, when not NULL: bit 0 sim01, bit 1 sim12, bit 2 sim20, bits 4..6 the tracks'
// activity.  Returns the number of vectors (0 .. 3).  The averages are float32, per component.
MACCDOA_HD int unify_cell(const float *act, const float *v, float sed_threshold, double cos_unify, float *out, int *flags)
{
    bool a[N_TRACKS];
    for (int n = 0; n < N_TRACKS; n++) a[n] = seld_decode::is_active(act[n], sed_threshold);
    const bool s01 = similar(a[0], a[1], v, v + 3, cos_unify), s12 = similar(a[1], a[2], v + 3, v + 6, cos_unify),
               s20 = similar(a[2], a[0], v + 6, v, cos_unify);
    if (flags) *flags = (int)s01 | (int)s12 << 1 | (int)s20 << 2 | (int)a[0] << 4 | (int)a[1] << 5 | (int)a[2] << 6;
    const int n_sim = (int)s01 + (int)s12 + (int)s20;
    int n_out = 0;
    if (n_sim == 0) {
        for (int n = 0; n < N_TRACKS; n++)
            if (a[n]) {
                for (int c = 0; c < 3; c++) out[n_out * 3 + c] = v[n * 3 + c];
                n_out++;
            }
    } else if (n_sim == 1) {
        const int i = s12 ? 1 : 0, j = s01 ? 1 : 2, other = 3 - i - j;          // the pair (i < j) and the third track
        for (int g = 0; g < 2; g++) {                                           // groups by their lowest track: min(i, other) first
            const bool pair = (g == 0) == (i < other);
            if (pair) {
                for (int c = 0; c < 3; c++) out[n_out * 3 + c] = (v[i * 3 + c] + v[j * 3 + c]) / 2.0f;
                n_out++;
            } else if (a[other]) {
                for (int c = 0; c < 3; c++) out[n_out * 3 + c] = v[other * 3 + c];
                n_out++;
            }
        }
    } else {
        for (int c = 0; c < 3; c++) out[c] = ((v[c] + v[3 + c]) + v[6 + c]) / 3.0f;
        n_out = 1;
    }
    return n_out;
}

} // namespace multi_accdoa
