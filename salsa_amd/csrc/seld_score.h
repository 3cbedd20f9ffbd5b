// seld_score.h -- per-element statements of salsa_nn_seld_score (seld_score.hip): the great-circle distance of two integer-degree
// directions, the pairing of one (class, frame) cell, the bookkeeping of one class of a segment and the record of the segment;
// behind them the per-class record of the SELD 2022 metric (salsa_nn_seld_score2022; tests/hostemu/score2022_emu.cpp, SeldMetrics2022)
// and the same three for the SELD 2020 metric (salsa_nn_seld_score2020; tests/hostemu/score2020_emu.cpp, SeldMetrics2020).
// Host + device inline functions over plain arrays (LDS on the device); the same header compiles with g++
// (tests/hostemu/score_emu.cpp), so the CPU suite holds every statement to crnn/metrics.py::SeldMetrics.  That host build is a test
// harness, never a fallback of the product.
//
// Reference semantics (paths relative to the upstream repository; crnn/metrics.py is the restatement golden g12 pins to them):
//   metrics/SELD2021_evaluation_metrics.py:81-195  SELDMetrics.update_seld_scores: per 1-s segment and class, DOAs of common frames
//                                                  are paired by minimum total distance, distances averaged per reference slot
//   metrics/SELD2021_evaluation_metrics.py:198-209 distance_between_spherical_coordinates_rad
//
// Everything is float64 with contraction off.  The device's sin / cos / acos are not glibc's bit for bit, so the statements never
// DECIDE inside `margin` of a boundary: a cell whose best two pairings cost the same to within margin, or a slot average within
// margin of the threshold, marks the segment DOUBT and the exact host code scores it (crnn/score.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SCORE_HD __host__ __device__ __forceinline__
#else
#define SCORE_HD inline
#endif

namespace seld_score {

constexpr int MAX_DOAS = 4, MAX_CLASSES = 32, MAX_RATE = 32, MAX_CELLS = MAX_CLASSES * MAX_RATE, N_COUNTERS = 10;
constexpr int COUNT_SAT = MAX_DOAS + 1;                 // a cell's count saturates here: "more than MAX_DOAS" is all that is asked of it
enum { C_TP, C_FP, C_FN, C_S, C_D, C_I, C_NREF, C_DE_TP, C_DE_FP, C_DE_FN };
enum { SCORED = 0, DOUBT = 1, REFUSED = 2 };

// a cell's DOAs as they arrive, (azimuth, elevation) packed into 32 bits; the pairing replaces them by the matched distances of the
// (at most 4) reference slots: 32 bytes either way, read into registers before they are overwritten
union Cell {
    struct { int32_t g[MAX_DOAS], p[MAX_DOAS]; } in;
    double cost[MAX_DOAS];
};

struct ClassResult {
    int counters[N_COUNTERS];                           // C_S, C_D, C_I stay 0: they are formed per segment
    int seg_fp, seg_fn, n_avg, flags;                   // flags: bit 0 doubt, bit 1 refused
    double avg[MAX_DOAS];                               // the slot averages in the order SeldMetrics adds them to total_DE
};

SCORE_HD int n_segments(int n_frames, int label_rate) { return (n_frames + label_rate - 1) / label_rate; }

SCORE_HD int32_t pack_doa(int16_t azimuth, int16_t elevation) { return (int32_t)((uint32_t)(uint16_t)azimuth | ((uint32_t)(uint16_t)elevation << 16)); }
SCORE_HD int doa_azimuth(int32_t d) { return (int16_t)((uint32_t)d & 0xffffu); }
SCORE_HD int doa_elevation(int32_t d) { return (int16_t)((uint32_t)d >> 16); }

// the cell of a row in segment `seg`: class * label_rate + frame in segment, or -1 when the row is not the segment's.  Frames
// outside 0 .. n_seg * label_rate - 1 belong to no segment (segment < 0 or >= n_seg never matches); classes outside are never read.
SCORE_HD int cell_of(int frame, int cls, int seg, int label_rate, int n_classes)
{
    if (frame < 0 || cls < 0 || cls >= n_classes) return -1;
    if (frame / label_rate != seg) return -1;
    return cls * label_rate + frame % label_rate;
}

// metrics.py::angular_distance_deg, statement for statement: v * pi / 180 per angle, sin sin + cos cos cos(|da|), clip, acos * 180 / pi
SCORE_HD double distance_deg(int azi1, int ele1, int azi2, int ele2)
{
#if defined(__HIPCC__) // (the g++ harness is built with -ffp-contract=off)
#pragma clang fp contract(off)
#endif
    const double pi = 3.141592653589793;
    const double a1 = (double)azi1 * pi / 180.0, e1 = (double)ele1 * pi / 180.0, a2 = (double)azi2 * pi / 180.0, e2 = (double)ele2 * pi / 180.0;
    double d = sin(e1) * sin(e2) + cos(e1) * cos(e2) * cos(fabs(a1 - a2));
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);
    return acos(d) * 180.0 / pi;
}

// One cell with 1 .. 4 DOAs on both sides: the minimum-total-cost injective map of the smaller side into the larger, by brute force
// over the at most 24 maps.  cost[r] receives the distance of every matched reference slot r; returns the mask of matched slots.
// *doubt: another map costs within `margin` of the best (scipy's choice among them is not ours to guess).
SCORE_HD unsigned pair_cell(const int32_t *g, int ng, const int32_t *p, int np, double margin, double *cost, bool *doubt)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    double c[MAX_DOAS][MAX_DOAS];
    for (int r = 0; r < ng; r++)
        for (int q = 0; q < np; q++) c[r][q] = distance_deg(doa_azimuth(g[r]), doa_elevation(g[r]), doa_azimuth(p[q]), doa_elevation(p[q]));
    const bool g_small = ng <= np;
    const int small = g_small ? ng : np, large = g_small ? np : ng;
    int n_codes = 1;
    for (int i = 0; i < small; i++) n_codes *= large;                        // digit i of a code (base `large`): where item i of the smaller side goes
    double best = INFINITY, second = INFINITY;
    int best_code = 0;
    for (int code = 0; code < n_codes; code++) {
        unsigned used = 0;
        double total = 0.0;
        bool injective = true;
        for (int i = 0, rest = code; i < small; i++, rest /= large) {
            const int to = rest % large;
            if (used >> to & 1u) injective = false;
            used |= 1u << to;
            total += g_small ? c[i][to] : c[to][i];
        }
        if (!injective) continue;
        if (total < best) {
            second = best;
            best = total;
            best_code = code;
        } else if (total < second) {
            second = total;
        }
    }
    *doubt = second - best <= margin;                                        // (one map only: inf - best, never in doubt)
    unsigned matched = 0;
    for (int i = 0, rest = best_code; i < small; i++, rest /= large) {
        const int to = rest % large, r = g_small ? i : to, q = g_small ? to : i;
        cost[r] = c[r][q];
        matched |= 1u << r;
    }
    return matched;
}

// One class of one segment, from its label_rate cells (the arrays point at the class's first cell): gcnt / pcnt the saturated DOA
// counts, matched / cell_doubt / cells[].cost what pair_cell left for the cells with both sides present, gfirst the arrival index
// of a reference cell's first row.  SeldMetrics walks the reference frames in the order they first arrived and keeps the slots in
// the order they were first matched; sums and averages follow that order so that they round as SeldMetrics' do.
// sel, when not NULL: frame f's pairing (cells, matched, cell_doubt) is entry sel[f], not f -- the threshold sweep (seld_sweep.h) keeps
// one pairing per distinct predicted set of a cell and picks per candidate; the counts and gfirst stay per frame.
SCORE_HD void score_class_sel(const Cell *cells, const uint8_t *gcnt, const uint8_t *pcnt, const uint8_t *matched, const uint8_t *cell_doubt,
                              const int *gfirst, const uint8_t *sel, int label_rate, double threshold, double margin, ClassResult *out)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    ClassResult res;
    for (int k = 0; k < N_COUNTERS; k++) res.counters[k] = 0;
    res.seg_fp = res.seg_fn = res.n_avg = res.flags = 0;
    for (int k = 0; k < MAX_DOAS; k++) res.avg[k] = 0.0;
    int n_g = 0, n_p = 0;
    for (int f = 0; f < label_rate; f++) {
        n_g = gcnt[f] > n_g ? gcnt[f] : n_g;
        n_p = pcnt[f] > n_p ? pcnt[f] : n_p;
    }
    if (n_g > MAX_DOAS || n_p > MAX_DOAS) {
        res.flags = 2;
        *out = res;
        return;
    }
    res.counters[C_NREF] = n_g;
    if (n_g && n_p) {
        double sum[MAX_DOAS] = {0.0, 0.0, 0.0, 0.0};
        int n[MAX_DOAS] = {0, 0, 0, 0}, order[MAX_DOAS] = {0, 0, 0, 0}, n_slots = 0;
        for (int prev = -1;;) {                                              // reference frames by first arrival (label_rate <= 32 of them)
            int f = -1;
            for (int k = 0; k < label_rate; k++)
                if (gcnt[k] && gfirst[k] > prev && (f < 0 || gfirst[k] < gfirst[f])) f = k;
            if (f < 0) break;
            prev = gfirst[f];
            if (!pcnt[f]) continue;
            const int e = sel ? sel[f] : f;
            if (cell_doubt[e]) res.flags |= 1;
            for (int r = 0; r < MAX_DOAS; r++) {
                if (!(matched[e] >> r & 1)) continue;
                if (!n[r]) order[n_slots++] = r;
                sum[r] += cells[e].cost[r];
                n[r]++;
            }
        }
        if (!n_slots) {                                                      // no common frame: the PREDICTED count is booked as misses
            res.counters[C_FN] += n_p;
            res.counters[C_DE_FN] += n_p;
            res.seg_fn += n_p;
        } else {
            for (int k = 0; k < n_slots; k++) {
                const int r = order[k];
                const double avg = sum[r] / (double)n[r];
                res.avg[res.n_avg++] = avg;
                res.counters[C_DE_TP]++;
                if (fabs(avg - threshold) <= margin) res.flags |= 1;
                if (avg <= threshold) {
                    res.counters[C_TP]++;
                } else {
                    res.counters[C_FP]++;
                    res.seg_fp++;
                }
            }
            if (n_p > n_g) {
                res.counters[C_FP] += n_p - n_g;
                res.counters[C_DE_FP] += n_p - n_g;
                res.seg_fp += n_p - n_g;
            } else if (n_p < n_g) {
                res.counters[C_FN] += n_g - n_p;
                res.counters[C_DE_FN] += n_g - n_p;
                res.seg_fn += n_g - n_p;
            }
        }
    } else if (n_g) {
        res.counters[C_FN] += n_g;
        res.counters[C_DE_FN] += n_g;
        res.seg_fn += n_g;
    } else if (n_p) {
        res.counters[C_FP] += n_p;
        res.counters[C_DE_FP] += n_p;
        res.seg_fp += n_p;
    }
    *out = res;
}

SCORE_HD void score_class(const Cell *cells, const uint8_t *gcnt, const uint8_t *pcnt, const uint8_t *matched, const uint8_t *cell_doubt,
                          const int *gfirst, int label_rate, double threshold, double margin, ClassResult *out)
{
    score_class_sel(cells, gcnt, pcnt, matched, cell_doubt, gfirst, nullptr, label_rate, threshold, margin, out);
}

// The record of one segment from its classes, in class order: total_DE is ONE running sum over every slot average, as SeldMetrics
// keeps it.  A segment in doubt or refused carries zero counters (the host scores it whole).
SCORE_HD void segment_record(const ClassResult *res, int n_classes, int *counters, double *total_de, int *status)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    int cnt[N_COUNTERS], seg_fp = 0, seg_fn = 0, flags = 0;
    double total = 0.0;
    for (int k = 0; k < N_COUNTERS; k++) cnt[k] = 0;
    for (int c = 0; c < n_classes; c++) {
        for (int k = 0; k < N_COUNTERS; k++) cnt[k] += res[c].counters[k];
        for (int k = 0; k < res[c].n_avg; k++) total += res[c].avg[k];
        seg_fp += res[c].seg_fp;
        seg_fn += res[c].seg_fn;
        flags |= res[c].flags;
    }
    cnt[C_S] = seg_fp < seg_fn ? seg_fp : seg_fn;
    cnt[C_D] = seg_fn > seg_fp ? seg_fn - seg_fp : 0;
    cnt[C_I] = seg_fp > seg_fn ? seg_fp - seg_fn : 0;
    const int st = flags & 2 ? REFUSED : (flags & 1 ? DOUBT : SCORED);
    for (int k = 0; k < N_COUNTERS; k++) counters[k] = st == SCORED ? cnt[k] : 0;
    *total_de = st == SCORED ? total : 0.0;
    *status = st;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The class-wise SELD 2022 metric (salsa_nn_seld_score2022; crnn/metrics.py::SeldMetrics2022, the project's own restatement of the
// public DCASE 2022 metric: DESIGN.md section 9t).  The pairing and the bookkeeping are the 2021 ones, score_class above; only where
// the bookkeeping lands changes: the class axis is kept, and a slot average above the threshold is a false positive of its own kind
// (FP_spatial), no longer part of FP.  So per class FP == DE_FP, FN == DE_FN and FP_spatial == DE_TP - TP, and five counters are
// all a class of a segment has to carry.
constexpr int N_CLASS_COUNTERS = 5;
enum { K_TP, K_NREF, K_DE_TP, K_DE_FP, K_DE_FN };

// The segment's own part, from its classes in class order: S, D, I from seg_fp / seg_fn over all classes (a slot average above the
// threshold still counts in seg_fp), and the status by segment_record's rules.  A segment in doubt or refused carries zeros.
SCORE_HD void segment_sdi2022(const ClassResult *res, int n_classes, int *sdi, int *status)
{
    int seg_fp = 0, seg_fn = 0, flags = 0;
    for (int c = 0; c < n_classes; c++) {
        seg_fp += res[c].seg_fp;
        seg_fn += res[c].seg_fn;
        flags |= res[c].flags;
    }
    const int st = flags & 2 ? REFUSED : (flags & 1 ? DOUBT : SCORED);
    sdi[0] = st == SCORED ? (seg_fp < seg_fn ? seg_fp : seg_fn) : 0;
    sdi[1] = st == SCORED && seg_fn > seg_fp ? seg_fn - seg_fp : 0;
    sdi[2] = st == SCORED && seg_fp > seg_fn ? seg_fp - seg_fn : 0;
    *status = st;
}

// One class of a segment of status `st`: the five independent counters and the class's share of total_DE, its slot averages added
// from 0.0 in the order score_class left them in avg[] -- what SeldMetrics2022 adds to total_DE[c] for the segment alone.
SCORE_HD void class_record2022(const ClassResult *res, int st, int *counters, double *class_de)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    double total = 0.0;
    for (int k = 0; k < res->n_avg; k++) total += res->avg[k];
    const bool scored = st == SCORED;
    counters[K_TP] = scored ? res->counters[C_TP] : 0;
    counters[K_NREF] = scored ? res->counters[C_NREF] : 0;
    counters[K_DE_TP] = scored ? res->counters[C_DE_TP] : 0;
    counters[K_DE_FP] = scored ? res->counters[C_DE_FP] : 0;
    counters[K_DE_FN] = scored ? res->counters[C_DE_FN] : 0;
    *class_de = scored ? total : 0.0;
}

// The per-class record of one segment: class_counters [n_classes][5], class_de [n_classes], sdi [3] and the status (the kernel
// gives class_record2022 a thread per class; this is the same two statements in a row)
SCORE_HD void segment_record2022(const ClassResult *res, int n_classes, int *class_counters, double *class_de, int *sdi, int *status)
{
    segment_sdi2022(res, n_classes, sdi, status);
    for (int c = 0; c < n_classes; c++) class_record2022(res + c, *status, class_counters + c * N_CLASS_COUNTERS, class_de + c);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The SELD 2020 metric (salsa_nn_seld_score2020; crnn/metrics.py::SeldMetrics2020 is the restatement golden g29 pins to the reference):
//   metrics/SELD2020_evaluation_metrics.py:159-229  SELDMetrics.update_seld_scores: per 1-s segment and class, PRESENCE counts; the
//                                                   reference frames in ascending order, each common frame costing the least total
//                                                   distance of pairing the smaller side into the larger; the mean cost decides
//   metrics/SELD2020_evaluation_metrics.py:266-294  least_distance_between_gt_pred
// Only the VALUE of a frame's minimum enters, never which map attains it, so a rival map of nearly equal cost is no doubt here: the
// one close call is a class average within `margin` of the threshold.
enum { C20_TP, C20_FP, C20_FN, C20_TN, C20_S, C20_D, C20_I, C20_NREF, C20_NSYS, C20_DE_TP };

// One cell with 1 .. 4 DOAs on both sides: the least total cost over the at most 24 injective maps of the smaller side into the
// larger.  The best map's costs are added in reference-slot order, the order of cost_mat[row_ind, col_ind].sum().
SCORE_HD double cell_cost2020(const int32_t *g, int ng, const int32_t *p, int np)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    double c[MAX_DOAS][MAX_DOAS];
    for (int r = 0; r < ng; r++)
        for (int q = 0; q < np; q++) c[r][q] = distance_deg(doa_azimuth(g[r]), doa_elevation(g[r]), doa_azimuth(p[q]), doa_elevation(p[q]));
    const bool g_small = ng <= np;
    const int small = g_small ? ng : np, large = g_small ? np : ng;
    int n_codes = 1;
    for (int i = 0; i < small; i++) n_codes *= large;                        // digit i of a code (base `large`): where item i of the smaller side goes
    double best = INFINITY;
    int best_code = 0;
    for (int code = 0; code < n_codes; code++) {
        unsigned used = 0;
        double total = 0.0;
        bool injective = true;
        for (int i = 0, rest = code; i < small; i++, rest /= large) {
            const int to = rest % large;
            if (used >> to & 1u) injective = false;
            used |= 1u << to;
            total += g_small ? c[i][to] : c[to][i];
        }
        if (injective && total < best) {
            best = total;
            best_code = code;
        }
    }
    int col[MAX_DOAS] = {-1, -1, -1, -1};                                    // the predicted DOA of every matched reference slot
    for (int i = 0, rest = best_code; i < small; i++, rest /= large) {
        const int to = rest % large;
        col[g_small ? i : to] = g_small ? to : i;
    }
    double total = 0.0;
    for (int r = 0; r < ng; r++)
        if (col[r] >= 0) total += c[r][col[r]];
    return total;
}

// One class of one segment from its label_rate cells: gcnt / pcnt the saturated DOA counts, cells[f].cost[0] what cell_cost2020
// gave for the cells with both sides present.  The frames are walked in ascending order, as dcase_utils.segment_labels leaves them
// whatever the order of the rows.  counters: the C20_ ones (S, D, I stay 0); seg_fp / seg_fn the segment's loc_FP / loc_FN.
SCORE_HD void score_class2020(const Cell *cells, const uint8_t *gcnt, const uint8_t *pcnt, int label_rate, double threshold, double margin,
                              ClassResult *out)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    ClassResult res;
    for (int k = 0; k < N_COUNTERS; k++) res.counters[k] = 0;
    res.seg_fp = res.seg_fn = res.n_avg = res.flags = 0;
    for (int k = 0; k < MAX_DOAS; k++) res.avg[k] = 0.0;
    int n_g = 0, n_p = 0, n = 0;
    for (int f = 0; f < label_rate; f++) {
        n_g = gcnt[f] > n_g ? gcnt[f] : n_g;
        n_p = pcnt[f] > n_p ? pcnt[f] : n_p;
    }
    if (n_g > MAX_DOAS || n_p > MAX_DOAS) {                                  // (such a cell has no cost)
        res.flags = 2;
        *out = res;
        return;
    }
    double total = 0.0;
    for (int f = 0; f < label_rate; f++)
        if (gcnt[f] && pcnt[f]) {
            total += cells[f].cost[0];
            n++;
        }
    res.counters[C20_NREF] = n_g ? 1 : 0;
    res.counters[C20_NSYS] = n_p ? 1 : 0;
    if (n_g && n_p) {
        if (!n) {                                                            // no common frame
            res.counters[C20_FN] = res.seg_fn = 1;
        } else {
            const double avg = total / (double)n;
            res.avg[res.n_avg++] = avg;
            res.counters[C20_DE_TP] = 1;
            if (fabs(avg - threshold) <= margin) res.flags |= 1;
            if (avg <= threshold) res.counters[C20_TP] = 1;
            else res.counters[C20_FN] = res.seg_fn = 1;
        }
    } else if (n_g) {
        res.counters[C20_FN] = res.seg_fn = 1;
    } else if (n_p) {
        res.counters[C20_FP] = res.seg_fp = 1;
    } else {
        res.counters[C20_TN] = 1;
    }
    *out = res;
}

// The record of one segment from its classes, in class order: total_DE is ONE running sum over the class averages, as
// SeldMetrics2020 keeps it.  A segment in doubt or refused carries zero counters (the host scores it whole).
SCORE_HD void segment_record2020(const ClassResult *res, int n_classes, int *counters, double *total_de, int *status)
{
#if defined(__HIPCC__)
#pragma clang fp contract(off)
#endif
    int cnt[N_COUNTERS], seg_fp = 0, seg_fn = 0, flags = 0;
    double total = 0.0;
    for (int k = 0; k < N_COUNTERS; k++) cnt[k] = 0;
    for (int c = 0; c < n_classes; c++) {
        for (int k = 0; k < N_COUNTERS; k++) cnt[k] += res[c].counters[k];
        for (int k = 0; k < res[c].n_avg; k++) total += res[c].avg[k];
        seg_fp += res[c].seg_fp;
        seg_fn += res[c].seg_fn;
        flags |= res[c].flags;
    }
    cnt[C20_S] = seg_fp < seg_fn ? seg_fp : seg_fn;
    cnt[C20_D] = seg_fn > seg_fp ? seg_fn - seg_fp : 0;
    cnt[C20_I] = seg_fp > seg_fn ? seg_fp - seg_fn : 0;
    const int st = flags & 2 ? REFUSED : (flags & 1 ? DOUBT : SCORED);
    for (int k = 0; k < N_COUNTERS; k++) counters[k] = st == SCORED ? cnt[k] : 0;
    *total_de = st == SCORED ? total : 0.0;
    *status = st;
}

} // namespace seld_score
