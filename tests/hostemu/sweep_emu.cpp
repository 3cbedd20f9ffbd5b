// tests/hostemu/sweep_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/seld_sweep.h (the per-element statements of
// salsa_nn_seld_sweep: one decode and pairing per distinct predicted set of a cell, then the class bookkeeping per candidate).  TEST
// INFRASTRUCTURE ONLY: tests/test_threshold_sweep_cpu.py builds it with g++ -ffp-contract=off (and -fno-builtin-sin -fno-builtin-cos,
// as score2022_emu.cpp is built) and holds the records to crnn/calibrate.py::sweep_host where there is no GPU.  The product never
// loads it and has no CPU path.
#include <vector>
#include "../../salsa_amd/csrc/seld_sweep.h"
using namespace seld_score;

extern "C" {

// one file: act [n_frames][nc | 3 C], xyz [n_frames][3 nc | 9 C], thresholds [K][n_classes], gt [n_gt][4] -> class_counters
// [n_seg][K][n_classes][5], class_de [n_seg][K][n_classes], status [n_seg][K][n_classes]; the kernel's walk, serially: the reference
// rows binned in arrival order, the classes in groups of seld_sweep::group_classes, an entry per (class, predicted set, frame), then
// every (candidate, class).  The launcher's argument checks are restated by the caller.
void emu_sweep_file(const float *act, const float *xyz, int n_frames, int n_classes, int multi, double cos_unify, const float *thresholds, int K,
                    const int16_t *gt, int n_gt, int label_rate, double doa_threshold, double margin, int *class_counters, double *class_de,
                    int *status)
{
    const int n_seg = n_segments(n_frames, label_rate), n_cells = n_classes * label_rate;
    const int sets = seld_sweep::n_sets(multi), tracks = seld_sweep::n_tracks(multi), per_class = sets * label_rate;
    const int group = seld_sweep::group_classes(n_classes, label_rate, multi);
    for (int seg = 0; seg < n_seg; seg++) {
        std::vector<int32_t> g(n_cells * MAX_DOAS, 0);
        std::vector<uint8_t> gcnt(n_cells, 0);
        std::vector<int> gfirst(n_cells, 0);
        for (int i = 0; i < n_gt; i++) {
            const int cell = cell_of(gt[4 * i], gt[4 * i + 1], seg, label_rate, n_classes);
            if (cell < 0) continue;
            const int slot = gcnt[cell];
            if (slot < MAX_DOAS) g[cell * MAX_DOAS + slot] = pack_doa(gt[4 * i + 2], gt[4 * i + 3]);
            if (slot == 0) gfirst[cell] = i;
            gcnt[cell] = (uint8_t)(slot + 1 < COUNT_SAT ? slot + 1 : COUNT_SAT);
        }
        std::vector<Cell> cells(seld_sweep::ENTRIES);
        std::vector<uint8_t> npred(seld_sweep::ENTRIES), matched(seld_sweep::ENTRIES), cell_doubt(seld_sweep::ENTRIES);
        std::vector<float> acts(seld_sweep::ENTRIES);
        for (int c0 = 0; c0 < n_classes; c0 += group) {
            const int gc = n_classes - c0 < group ? n_classes - c0 : group;
            for (int e = 0; e < gc * per_class; e++) {
                const int ci = e / per_class, rest = e - ci * per_class, set = rest / label_rate + 1, f = rest - (set - 1) * label_rate;
                const int cls = c0 + ci, cell = cls * label_rate + f, frame = seg * label_rate + f;
                const bool in_file = frame < n_frames;
                float a[3] = {0.f, 0.f, 0.f}, v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (in_file)
                    seld_sweep::load_cell(act + (size_t)frame * tracks * n_classes, xyz + (size_t)frame * 3 * tracks * n_classes, n_classes, cls, multi, a, v);
                if (set == 1)
                    for (int n = 0; n < tracks; n++) acts[(ci * label_rate + f) * tracks + n] = in_file ? a[n] : __builtin_nanf("");
                seld_sweep::pair_entry(&g[cell * MAX_DOAS], gcnt[cell], in_file, v, multi, set, cos_unify, margin, &cells[e], &npred[e], &matched[e],
                                       &cell_doubt[e]);
            }
            for (int it = 0; it < K * gc; it++) {
                const int k = it / gc, ci = it - k * gc, cls = c0 + ci, at = ci * per_class;
                const size_t o = ((size_t)seg * K + k) * n_classes + cls;
                seld_sweep::sweep_class(cells.data() + at, gcnt.data() + cls * label_rate, npred.data() + at, matched.data() + at,
                                        cell_doubt.data() + at, gfirst.data() + cls * label_rate, acts.data() + ci * label_rate * tracks, tracks,
                                        thresholds[k * n_classes + cls], label_rate, doa_threshold, margin, class_counters + o * N_CLASS_COUNTERS,
                                        class_de + o, status + o);
            }
        }
    }
}
}
