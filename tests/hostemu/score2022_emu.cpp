// tests/hostemu/score2022_emu.cpp -- CPU unit-test harness for the class-wise SELD 2022 statements of salsa_amd/csrc/seld_score.h
// (the per-element statements of salsa_nn_seld_score2022: the 2021 pairing and class bookkeeping, then segment_record2022).  TEST
// INFRASTRUCTURE ONLY: tests/test_seld_score2022_cpu.py builds it with g++ -ffp-contract=off (and -fno-builtin-sin -fno-builtin-cos:
// no merged sincos calls, so that every value is the C library's sin or cos) and holds the records to
// crnn/metrics.py::SeldMetrics2022 where there is no GPU.  The product never loads it and has no CPU path.
#include <vector>
#include "../../salsa_amd/csrc/seld_score.h"
using namespace seld_score;

namespace {

// one side's rows [count][4] into the segment's cells, serially, what the kernel's tiles do: arrival order, saturated counts
void bin_rows(bool is_gt, const int16_t *rows, int count, int seg, int label_rate, int n_classes, Cell *cells, uint8_t *cnt, int *gfirst)
{
    for (int i = 0; i < count; i++) {
        const int cell = cell_of(rows[4 * i], rows[4 * i + 1], seg, label_rate, n_classes);
        if (cell < 0) continue;
        const int slot = cnt[cell];
        if (slot < MAX_DOAS) (is_gt ? cells[cell].in.g : cells[cell].in.p)[slot] = pack_doa(rows[4 * i + 2], rows[4 * i + 3]);
        if (is_gt && slot == 0) gfirst[cell] = i;
        cnt[cell] = (uint8_t)(slot + 1 < COUNT_SAT ? slot + 1 : COUNT_SAT);
    }
}

} // namespace

extern "C" {

// one file: class_counters [n_seg][n_classes][5], class_de [n_seg][n_classes], sdi [n_seg][3], status [n_seg]; the launcher's
// argument checks are restated by the caller
void emu_score2022_file(const int16_t *pred, int n_pred, const int16_t *gt, int n_gt, int n_frames, int label_rate, int n_classes,
                        double threshold, double margin, int *class_counters, double *class_de, int *sdi, int *status)
{
    const int n_seg = n_segments(n_frames, label_rate), n_cells = n_classes * label_rate;
    for (int seg = 0; seg < n_seg; seg++) {
        std::vector<Cell> cells(n_cells);
        std::vector<uint8_t> gcnt(n_cells, 0), pcnt(n_cells, 0), matched(n_cells, 0), cell_doubt(n_cells, 0);
        std::vector<int> gfirst(n_cells, 0);
        std::vector<ClassResult> res(n_classes);
        bin_rows(true, gt, n_gt, seg, label_rate, n_classes, cells.data(), gcnt.data(), gfirst.data());
        bin_rows(false, pred, n_pred, seg, label_rate, n_classes, cells.data(), pcnt.data(), nullptr);
        for (int c = 0; c < n_cells; c++) {
            const int ng = gcnt[c], np = pcnt[c];
            if (ng < 1 || np < 1 || ng > MAX_DOAS || np > MAX_DOAS) continue;
            int32_t g[MAX_DOAS], p[MAX_DOAS];
            double cost[MAX_DOAS] = {0.0, 0.0, 0.0, 0.0};
            for (int k = 0; k < MAX_DOAS; k++) {
                g[k] = cells[c].in.g[k];
                p[k] = cells[c].in.p[k];
            }
            bool doubt;
            matched[c] = (uint8_t)pair_cell(g, ng, p, np, margin, cost, &doubt);
            for (int k = 0; k < MAX_DOAS; k++) cells[c].cost[k] = cost[k];
            cell_doubt[c] = doubt ? 1 : 0;
        }
        for (int c = 0; c < n_classes; c++) {
            const int at = c * label_rate;
            score_class(cells.data() + at, gcnt.data() + at, pcnt.data() + at, matched.data() + at, cell_doubt.data() + at, gfirst.data() + at,
                        label_rate, threshold, margin, &res[c]);
        }
        segment_record2022(res.data(), n_classes, class_counters + seg * n_classes * N_CLASS_COUNTERS, class_de + seg * n_classes, sdi + seg * 3,
                           status + seg);
    }
}
}
