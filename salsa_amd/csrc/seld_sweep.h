// seld_sweep.h -- per-element statements of salsa_nn_seld_sweep (seld_sweep.hip): the class-wise SELD 2022
// counters of K candidate SED thresholds per class from ONE pass over a segment.  For the single-vector formats the direction of a
// (frame, class) does not depend on the threshold, and for Multi-ACCDOA the emitted set of a cell depends only on WHICH tracks are
// active (multi_accdoa.h, unify_cell): so a cell is decoded and paired once per distinct predicted set -- one for reg_xyz / accdoa,
// at most seven for three tracks -- and a candidate only selects, per frame, which of these pairings is present.  Decoding is
// seld_decode.h's and multi_accdoa.h's, pairing and class bookkeeping seld_score.h's (pair_cell, score_class_sel, class_record2022).
// Host + device inline functions over plain arrays (LDS on the device); the same header compiles with g++
// (tests/hostemu/sweep_emu.cpp), so the CPU suite holds every statement to crnn/calibrate.py::sweep_host.  That host build is a test
// harness, never a fallback of the product.
//
// Float64 with contraction off wherever seld_score.h is; the activity comparison stays float32 `activity >= threshold` (NaN on
// either side: inactive).  Doubt and refusal are per (segment, candidate, class): a class's counters depend on that class's rows alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include "multi_accdoa.h"
#include "seld_decode.h"
#include "seld_score.h"

namespace seld_sweep {

using seld_score::Cell;
using seld_score::MAX_DOAS;

constexpr int MAX_K = 64, N_SETS = 7;                   // candidates per class; non-empty active sets of three tracks
// pairing entries a workgroup keeps at a time: the classes of a segment are walked in groups of as many as fit (the 13 classes of a
// Multi-ACCDOA model at label rate 10 are 910 entries: one group; 32 x 32 single-vector cells need two)
constexpr int ENTRIES = 960;

SCORE_HD int n_sets(int multi) { return multi ? N_SETS : 1; }
SCORE_HD int n_tracks(int multi) { return multi ? multi_accdoa::N_TRACKS : 1; }

// classes per group: an entry per (class, predicted set, frame of the segment); at least 4 (32 frames x 7 sets)
SCORE_HD int group_classes(int n_classes, int label_rate, int multi)
{
    const int fit = ENTRIES / (label_rate * n_sets(multi));
    return n_classes < fit ? n_classes : fit;
}

// the activities a[tracks] and vectors v[tracks * 3 + axis] of class c from one frame's outputs: act [nc] / xyz [x | y | z] for the
// single-vector formats, act [3 C] / xyz [9 C] (pseudo-class n C + c per axis block) for Multi-ACCDOA
SCORE_HD void load_cell(const float *frame_act, const float *frame_xyz, int C, int c, int multi, float *a, float *v)
{
    const int tracks = n_tracks(multi);
    for (int n = 0; n < tracks; n++) {
        a[n] = frame_act[n * C + c];
        for (int k = 0; k < 3; k++) v[n * 3 + k] = frame_xyz[(tracks * k + n) * C + c];
    }
}

// the set of active tracks of a cell at one candidate, bit n = track n; 0: nothing is predicted
SCORE_HD int active_set(const float *a, int tracks, float threshold)
{
    int set = 0;
    for (int n = 0; n < tracks; n++) set |= (int)seld_decode::is_active(a[n], threshold) << n;
    return set;
}

// One entry: the (frame, class) cell with the tracks of `set` (1 .. 7; single-vector: 1) active, against the cell's ng reference
// DOAs g.  *npred: how many DOAs the decoder emits (unify_cell on the set; single-vector: 1) -- kept for every entry, the class's
// predicted count needs it where there is no reference; *matched / *doubt / cell->cost: pair_cell's, for 1 .. 4 references, else 0.
// in_file false (a frame of the last segment behind the file's end): nothing is predicted.
SCORE_HD void pair_entry(const int32_t *g, int ng, bool in_file, const float *v, int multi, int set, double cos_unify, double margin, Cell *cell,
                         uint8_t *npred, uint8_t *matched, uint8_t *doubt)
{
    *npred = *matched = *doubt = 0;
    if (!in_file) return;
    float out[9] = {v[0], v[1], v[2], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int n_out = 1;
    if (multi) {
        float on[multi_accdoa::N_TRACKS];
        for (int n = 0; n < multi_accdoa::N_TRACKS; n++) on[n] = (set >> n & 1) ? 1.0f : 0.0f;
        n_out = multi_accdoa::unify_cell(on, v, 0.5f, cos_unify, out, nullptr);   // (the set stands in for activity >= threshold)
    }
    *npred = (uint8_t)n_out;
    if (ng < 1 || ng > MAX_DOAS) return;                                          // (more than 4 references refuse the class in score_class)
    int32_t p[MAX_DOAS] = {0, 0, 0, 0};
    for (int q = 0; q < n_out; q++) {
        int16_t azimuth, elevation;
        seld_decode::xyz_to_angles(out[q * 3], out[q * 3 + 1], out[q * 3 + 2], &azimuth, &elevation);
        p[q] = seld_score::pack_doa(azimuth, elevation);
    }
    double cost[MAX_DOAS] = {0.0, 0.0, 0.0, 0.0};
    bool d;
    *matched = (uint8_t)seld_score::pair_cell(g, ng, p, n_out, margin, cost, &d);
    *doubt = d ? 1 : 0;
    for (int k = 0; k < MAX_DOAS; k++) cell->cost[k] = cost[k];
}

// the entry of (predicted set - 1, frame) among a class's n_sets * label_rate entries
SCORE_HD int entry_of(int set, int f, int label_rate) { return (set - 1) * label_rate + f; }

// One (candidate, class) of a segment: the class's entries (cells, npred, matched, cell_doubt: [n_sets][label_rate]), its reference
// counts gcnt / gfirst [label_rate], its activities act [label_rate][tracks] (NaN behind the file's end) and the candidate's
// threshold -> the five counters, the class's share of total_DE and the status of seld_score.h (0 scored, 1 doubt, 2 refused; the
// latter two carry zeros).
SCORE_HD void sweep_class(const Cell *cells, const uint8_t *gcnt, const uint8_t *npred, const uint8_t *matched, const uint8_t *cell_doubt,
                          const int *gfirst, const float *act, int tracks, float threshold, int label_rate, double doa_threshold, double margin,
                          int *counters, double *class_de, int *status)
{
    uint8_t pcnt[seld_score::MAX_RATE], sel[seld_score::MAX_RATE];
    for (int f = 0; f < label_rate; f++) {
        const int set = active_set(act + f * tracks, tracks, threshold);
        sel[f] = (uint8_t)(set ? entry_of(set, f, label_rate) : 0);               // (at most 6 * 32 + 31)
        pcnt[f] = set ? npred[sel[f]] : 0;
    }
    seld_score::ClassResult res;
    seld_score::score_class_sel(cells, gcnt, pcnt, matched, cell_doubt, gfirst, sel, label_rate, doa_threshold, margin, &res);
    const int st = res.flags & 2 ? seld_score::REFUSED : (res.flags & 1 ? seld_score::DOUBT : seld_score::SCORED);
    seld_score::class_record2022(&res, st, counters, class_de);
    *status = st;
}

} // namespace seld_sweep
