// tests/hostemu/score2020_emu.cpp -- CPU unit-test harness for the SELD 2020 statements of salsa_amd/csrc/seld_score.h (the
// per-element statements of salsa_nn_seld_score2020).  TEST INFRASTRUCTURE ONLY: tests/test_seld_score2020_cpu.py builds it with
// g++ -ffp-contract=off (and -fno-builtin-sin -fno-builtin-cos: no merged sincos calls, so that every value is the C library's sin
// or cos) and holds the records to crnn/metrics.py::SeldMetrics2020 where there is no GPU.  The product never loads it and has no
// CPU path.
#include <vector>
#include "../../salsa_amd/csrc/seld_score.h"
using namespace seld_score;

namespace {

// one side's rows [count][4] into the segment's cells, serially, what the kernel's tiles do: arrival order, saturated counts
void bin_rows(bool is_gt, const int16_t *rows, int count, int seg, int label_rate, int n_classes, Cell *cells, uint8_t *cnt)
{
    for (int i = 0; i < count; i++) {
        const int cell = cell_of(rows[4 * i], rows[4 * i + 1], seg, label_rate, n_classes);
        if (cell < 0) continue;
        const int slot = cnt[cell];
        if (slot < MAX_DOAS) (is_gt ? cells[cell].in.g : cells[cell].in.p)[slot] = pack_doa(rows[4 * i + 2], rows[4 * i + 3]);
        cnt[cell] = (uint8_t)(slot + 1 < COUNT_SAT ? slot + 1 : COUNT_SAT);
    }
}

} // namespace

extern "C" {

// one file: counters [n_seg][10], total_de [n_seg], status [n_seg]; the launcher's argument checks are restated by the caller
void emu_score2020_file(const int16_t *pred, int n_pred, const int16_t *gt, int n_gt, int n_frames, int label_rate, int n_classes,
                        double threshold, double margin, int *counters, double *total_de, int *status)
{
    const int n_seg = n_segments(n_frames, label_rate), n_cells = n_classes * label_rate;
    for (int seg = 0; seg < n_seg; seg++) {
        std::vector<Cell> cells(n_cells);
        std::vector<uint8_t> gcnt(n_cells, 0), pcnt(n_cells, 0);
        std::vector<ClassResult> res(n_classes);
        bin_rows(true, gt, n_gt, seg, label_rate, n_classes, cells.data(), gcnt.data());
        bin_rows(false, pred, n_pred, seg, label_rate, n_classes, cells.data(), pcnt.data());
        for (int c = 0; c < n_cells; c++) {
            const int ng = gcnt[c], np = pcnt[c];
            if (ng < 1 || np < 1 || ng > MAX_DOAS || np > MAX_DOAS) continue;
            int32_t g[MAX_DOAS], p[MAX_DOAS];
            for (int k = 0; k < MAX_DOAS; k++) {
                g[k] = cells[c].in.g[k];
                p[k] = cells[c].in.p[k];
            }
            cells[c].cost[0] = cell_cost2020(g, ng, p, np);
        }
        for (int c = 0; c < n_classes; c++) {
            const int at = c * label_rate;
            score_class2020(cells.data() + at, gcnt.data() + at, pcnt.data() + at, label_rate, threshold, margin, &res[c]);
        }
        segment_record2020(res.data(), n_classes, counters + seg * N_COUNTERS, total_de + seg, status + seg);
    }
}
}
