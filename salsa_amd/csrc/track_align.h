// track_align.h -- merging two Multi-ACCDOA forwards of one clip by aligning their tracks: the per-cell
// arithmetic of salsa_nn_tta_merge_multi and salsa_nn_chunk_merge_multi (track_align.hip).  Host + device inline functions; the same
// header compiles with g++ (tests/hostemu/track_align_emu.cpp), so every decision is checked against numpy on the CPU.  That host
// build is a test harness, never a fallback of the product.
//
// The reference has no Multi-ACCDOA; the definition is this project's.  The three tracks of a (frame, class) cell are an unordered
// set, so before two forwards are averaged one of them is permuted, cell by cell, onto the other:
//   align_cell   the permutation (multi_accdoa::source_of(3, cand, n): 012 021 102 120 201 210) of the incoming cell's tracks that is
//                closest to the anchor cell, by ADPIT's cost walk
//   merge_cell   one (clip, label frame, class) of the TTA / ensemble merge: every slab un-swapped (tta::unswap3, per track), every
//                slab after the first aligned to slab 0 ALONE, then tta::merge_one's fixed-order float32 sum and one division
//   file_cell    one (frame, class) of the chunk combine: seld_decode::file_value's walk with the fresh chunk aligned to the running
//                value before the pairwise average
// Layout: pseudo-class p = n C + c, blocks [x | y | z] of 3 C columns: component (axis a, track n, class c) of a row of 9 C columns is
// column (3 a + n) C + c, the activity of (track n, class c) column n C + c of a row of 3 C.
#pragma once
#include <math.h>
#include <stdint.h>
#include "multi_accdoa.h"
#include "tta.h"

#if defined(__HIPCC__) // (the g++ harness is built with -ffp-contract=off)
#pragma clang fp contract(off)
#endif

namespace track_align {

using multi_accdoa::N_TRACKS;
constexpr int N_CANDIDATES = 6;

// v[s * 3 + a] by selection (s is a run-time value: the cell stays in registers)
MACCDOA_HD float of_track(const float *v, int s, int a) { return s == 0 ? v[a] : s == 1 ? v[3 + a] : v[6 + a]; }

// R[n * 3 + a]: the anchor cell's track vectors, V[n * 3 + a]: the incoming cell's.  The cost of candidate pi is the sum over tracks
// (outer) and axes (inner) of (R[n][a] - V[pi(n)][a])^2, one running float64 sum without fma; the lowest index of the least cost wins:
// a later candidate replaces the current one only when strictly smaller, so a NaN cost never displaces candidate 0 and an exact tie
// keeps the lower index (the rule of multi_accdoa::adpit_item).
MACCDOA_HD int align_cell(const float *R, const float *V)
{
    int chosen = 0;
    double best = 0.0;
    TTA_UNROLL
    for (int cand = 0; cand < N_CANDIDATES; cand++) {
        double e = 0.0;
        TTA_UNROLL
        for (int n = 0; n < N_TRACKS; n++) {
            const int s = multi_accdoa::source_of(3, cand, n);
            TTA_UNROLL
            for (int a = 0; a < 3; a++) {
                const double d = (double)R[n * 3 + a] - (double)V[s * 3 + a];
                e = e + d * d;
            }
        }
        if (cand == 0 || e < best) {
            best = e;
            chosen = cand;
        }
    }
    return chosen;
}

// the length of one track vector as salsa_nn_accdoa_sed forms it (float32, no fma, correctly rounded square root)
MACCDOA_HD float track_activity(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// xyz: slab [N][cells][9 C]; cell = clip * L + label frame, c = real class.  out9[n * 3 + a]: the merged track vectors, act3[n] their
// lengths.  perm, when not NULL: [N][cells][C], receives the candidate chosen for every slab (0 for slab 0).
MACCDOA_HD void merge_cell(const float *xyz, int n_models, const tta::ids_t &ids, int n_var, int kind, int64_t cells, int C, int64_t cell,
                           int c, float *out9, float *act3, int *perm)
{
    float R[9], acc[9];
    int k = 0;
    for (int mi = 0; mi < n_models; mi++)
        for (int vi = 0; vi < n_var; vi++, k++) {
            int m[4];
            tta::variant_bits(kind, ids.v[vi], m);
            const int64_t at = (int64_t)k * cells + cell;
            const float *d = xyz + at * 9 * C + c;
            float V[9];
            TTA_UNROLL
            for (int n = 0; n < N_TRACKS; n++) {
                float x = d[(int64_t)n * C], y = d[(int64_t)(3 + n) * C], z = d[(int64_t)(6 + n) * C];
                tta::unswap3(x, y, z, kind == tta::KIND_FOA, m);
                V[n * 3] = x;
                V[n * 3 + 1] = y;
                V[n * 3 + 2] = z;
            }
            int cand = 0;
            if (k == 0) {
                TTA_UNROLL
                for (int j = 0; j < 9; j++) R[j] = acc[j] = V[j];
            } else {
                cand = align_cell(R, V);
                TTA_UNROLL
                for (int n = 0; n < N_TRACKS; n++) {
                    const int s = multi_accdoa::source_of(3, cand, n);
                    TTA_UNROLL
                    for (int a = 0; a < 3; a++) acc[n * 3 + a] = acc[n * 3 + a] + of_track(V, s, a);
                }
            }
            if (perm) perm[at * C + c] = cand;
        }
    const float fn = (float)k;
    TTA_UNROLL
    for (int j = 0; j < 9; j++) {
#if defined(__HIP_DEVICE_COMPILE__)
        out9[j] = __fdiv_rn(acc[j], fn);
#else
        out9[j] = acc[j] / fn;
#endif
    }
    TTA_UNROLL
    for (int n = 0; n < N_TRACKS; n++) act3[n] = track_activity(out9[n * 3], out9[n * 3 + 1], out9[n * 3 + 2]);
}

// one chunk's value of (frame `off` of chunk i, class c): activities a3[n] and vectors v9[n * 3 + a]
MACCDOA_HD void load_cell(const float *act, const float *xyz, int chunk_len, int C, int i, int off, int c, float *a3, float *v9)
{
    const int64_t row = (int64_t)i * chunk_len + off;
    const float *pa = act + row * 3 * C + c, *pv = xyz + row * 9 * C + c;
    TTA_UNROLL
    for (int n = 0; n < N_TRACKS; n++) {
        a3[n] = pa[(int64_t)n * C];
        TTA_UNROLL
        for (int a = 0; a < 3; a++) v9[n * 3 + a] = pv[(int64_t)(3 * a + n) * C];
    }
}

// one step of the walk (seld_decode::combine_step with the alignment in front of the average): chunk 0 and every frame behind the
// overlap overwrite; otherwise the fresh cell is aligned to the running one and v = (v + fresh[pi]) / 2.0f per component, the
// activities with the same pi
MACCDOA_HD void combine_cell(float *a3, float *v9, const float *fa, const float *fv, int i, int off, int overlap)
{
    if (i == 0 || off >= overlap) {
        TTA_UNROLL
        for (int n = 0; n < N_TRACKS; n++) a3[n] = fa[n];
        TTA_UNROLL
        for (int j = 0; j < 9; j++) v9[j] = fv[j];
        return;
    }
    const int cand = align_cell(v9, fv);
    TTA_UNROLL
    for (int n = 0; n < N_TRACKS; n++) {
        const int s = multi_accdoa::source_of(3, cand, n);
        a3[n] = (a3[n] + (s == 0 ? fa[0] : s == 1 ? fa[1] : fa[2])) / 2.0f;
        TTA_UNROLL
        for (int a = 0; a < 3; a++) v9[n * 3 + a] = (v9[n * 3 + a] + of_track(fv, s, a)) / 2.0f;
    }
}

// the combined file value of (frame, class c) from one file's chunks act [n_chunks][chunk_len][3 C] / xyz [..][9 C]: the chunks that
// hold the frame are visited in chunk order, the leftover chunk last (seld_decode::file_value's walk; the launcher checks
// n_chunks == expected_chunks and chunk_hop <= chunk_len <= n_frames when there is more than one chunk, so the first chunk over a
// frame always overwrites)
MACCDOA_HD void file_cell(const float *act, const float *xyz, int n_chunks, int chunk_len, int chunk_hop, int n_frames, int C, int frame,
                          int c, float *a3, float *v9)
{
    if (n_chunks == 1) {
        load_cell(act, xyz, chunk_len, C, 0, frame, c, a3, v9);
        return;
    }
    const int n_regular = (n_frames - chunk_len) / chunk_hop + 1, overlap = chunk_len - chunk_hop;
    const int lo = frame < chunk_len ? 0 : (frame - chunk_len) / chunk_hop + 1;
    const int hi = frame / chunk_hop < n_regular - 1 ? frame / chunk_hop : n_regular - 1;
    float fa[3], fv[9];
    TTA_UNROLL
    for (int n = 0; n < N_TRACKS; n++) a3[n] = 0.0f;
    TTA_UNROLL
    for (int j = 0; j < 9; j++) v9[j] = 0.0f;
    for (int i = lo; i <= hi; i++) {
        const int off = frame - i * chunk_hop;
        load_cell(act, xyz, chunk_len, C, i, off, c, fa, fv);
        combine_cell(a3, v9, fa, fv, i, off, overlap);
    }
    if (n_chunks > n_regular && frame >= n_frames - chunk_len) { // the leftover chunk, last in the walk
        const int off = frame - (n_frames - chunk_len);
        load_cell(act, xyz, chunk_len, C, n_chunks - 1, off, c, fa, fv);
        combine_cell(a3, v9, fa, fv, n_chunks - 1, off, overlap);
    }
}

} // namespace track_align
