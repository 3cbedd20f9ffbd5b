// seld_sweep.hip -- salsa_nn_seld_sweep (include/salsa_nn.h): the class-wise SELD 2022 counters of K candidate
// SED thresholds per class, from the combined file outputs and the ground-truth rows, in one launch.  The statements are
// seld_sweep.h's (which reuses seld_decode.h, multi_accdoa.h and seld_score.h); this file bins the reference rows and maps the work.
//
// One workgroup of 256 threads (4 waves) per (file, segment).  The reference rows are binned ONCE into the segment's cells in arrival
// order, by the rule seld_score.hip bins them with (seld_rows.h: tiles of 256 rows, one ballot per wave, no atomics).  Then the classes are walked in
// groups of as many as the entry table holds (seld_sweep.h, ENTRIES: one group at the usual 12 classes x 10 frames):
//   stage A, a thread per (class, predicted set, frame) entry: the cell is decoded and paired against its references once per
//            distinct predicted set (one for reg_xyz / accdoa, seven for the three tracks of Multi-ACCDOA) -- every distance, every
//            sin / cos / acos of the launch is here, and none of it depends on K;
//   stage B, a thread per (candidate, class), class fastest so that the record stores coalesce: the candidate's threshold against
//            the class's activities in LDS picks an entry per frame, and score_class_sel books the class.
// LDS (61 KB, two workgroups per CU): the cost table is read by stage B with a per-frame entry index, 32-byte entries of which only
// the matched slots are touched; the activities are 4 bytes per (frame, track).  Everything float64 is a few hundred distances per
// workgroup, as in seld_score.hip.  seld_sweep_file_sum_kernel adds each file's scored records in segment order, a thread per output
// element: no atomics anywhere, so two launches are bit-identical and a file's result does not depend on its batch.
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)
#include "seld_rows.h"
#include "seld_sweep.h"

namespace {

using namespace seld_score;
using seld_sweep::ENTRIES;

using seld_rows::DcaseRow;

constexpr int SWEEP_THREADS = seld_rows::BIN_THREADS;

struct SweepLds {
    Cell cells[ENTRIES];                                                       // 30 KB: the matched distances of every entry of the group
    int32_t g[MAX_CELLS][MAX_DOAS];                                            // 16 KB: the segment's reference DOAs, all classes
    int gfirst[MAX_CELLS];
    float act[ENTRIES];                                                        // [class of the group][frame][track]
    uint8_t gcnt[MAX_CELLS], npred[ENTRIES], matched[ENTRIES], cell_doubt[ENTRIES];
    seld_rows::BinScratch bin;
};
static_assert(sizeof(SweepLds) <= 64 * 1024, "static LDS of one workgroup; two per CU");
static_assert(seld_sweep::N_SETS * MAX_RATE * 4 <= ENTRIES, "at least four classes per group");
static_assert((seld_sweep::N_SETS - 1) * MAX_RATE + MAX_RATE - 1 <= 255, "a class's entry index fits sweep_class' uint8_t");

__global__ __launch_bounds__(SWEEP_THREADS) void seld_sweep_kernel(const float *__restrict__ act, const float *__restrict__ xyz, int n_in_frames,
                                                                   int n_frames, int n_classes, int multi, double cos_unify,
                                                                   const float *__restrict__ thresholds, int K,
                                                                   const DcaseRow *__restrict__ gt, const int *__restrict__ gt_counts,
                                                                   int gt_capacity, int n_seg, int label_rate, double doa_threshold,
                                                                   double margin, int *__restrict__ class_counters,
                                                                   double *__restrict__ class_de, int *__restrict__ status)
{
    __shared__ SweepLds s;
    const int tid = threadIdx.x, seg = blockIdx.x, n_cells = n_classes * label_rate;
    const size_t file = blockIdx.y, record = file * (size_t)n_seg + seg, out0 = record * K * n_classes;
    const int n_gt = gt_counts[file];
    if (n_gt < 0 || n_gt > gt_capacity) {                                      // (uniform) a count its slab cannot hold: nothing is read
        for (int i = tid; i < K * n_classes; i += SWEEP_THREADS) {
            for (int k = 0; k < N_CLASS_COUNTERS; k++) class_counters[(out0 + i) * N_CLASS_COUNTERS + k] = 0;
            class_de[out0 + i] = 0.0;
            status[out0 + i] = REFUSED;
        }
        return;
    }
    for (int c = tid; c < n_cells; c += SWEEP_THREADS) {
        s.gcnt[c] = 0;
        s.gfirst[c] = 0;
    }
    __syncthreads();
    seld_rows::bin_rows(s.bin, s.gcnt, gt + file * (size_t)gt_capacity, n_gt, seg, label_rate, n_classes,
                        [](int cell, int slot, int32_t doa, int row) {    // the reference side of seld_score.hip's cells (s: static LDS)
                            if (slot < MAX_DOAS) s.g[cell][slot] = doa;
                            if (slot == 0) s.gfirst[cell] = row;
                        });
    const int sets = seld_sweep::n_sets(multi), tracks = seld_sweep::n_tracks(multi), per_class = sets * label_rate;
    const int group = seld_sweep::group_classes(n_classes, label_rate, multi);
    const float *fact = act + file * (size_t)n_in_frames * tracks * n_classes;
    const float *fxyz = xyz + file * (size_t)n_in_frames * 3 * tracks * n_classes;
    for (int c0 = 0; c0 < n_classes; c0 += group) {                            // (uniform: every thread reaches the barriers)
        const int gc = n_classes - c0 < group ? n_classes - c0 : group;
        for (int e = tid; e < gc * per_class; e += SWEEP_THREADS) {            // stage A: e < group * per_class <= ENTRIES
            const int ci = e / per_class, rest = e - ci * per_class, set = rest / label_rate + 1, f = rest - (set - 1) * label_rate;
            const int cls = c0 + ci, cell = cls * label_rate + f, frame = seg * label_rate + f;
            const bool in_file = frame < n_frames;                             // (n_frames <= n_in_frames: nothing behind it is read)
            float a[3] = {0.f, 0.f, 0.f}, v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (in_file)
                seld_sweep::load_cell(fact + (size_t)frame * tracks * n_classes, fxyz + (size_t)frame * 3 * tracks * n_classes, n_classes, cls, multi, a, v);
            if (set == 1)                                                      // one thread of the cell keeps its activities
                for (int n = 0; n < tracks; n++) s.act[(ci * label_rate + f) * tracks + n] = in_file ? a[n] : __builtin_nanf("");
            int32_t g[MAX_DOAS];
            for (int k = 0; k < MAX_DOAS; k++) g[k] = s.g[cell][k];            // (slots behind gcnt are not read by pair_cell)
            seld_sweep::pair_entry(g, s.gcnt[cell], in_file, v, multi, set, cos_unify, margin, &s.cells[e], &s.npred[e], &s.matched[e],
                                   &s.cell_doubt[e]);
        }
        __syncthreads();
        for (int it = tid; it < K * gc; it += SWEEP_THREADS) {                 // stage B
            const int k = it / gc, ci = it - k * gc, cls = c0 + ci, at = ci * per_class;
            const size_t o = out0 + (size_t)k * n_classes + cls;
            seld_sweep::sweep_class(s.cells + at, s.gcnt + cls * label_rate, s.npred + at, s.matched + at, s.cell_doubt + at,
                                    s.gfirst + cls * label_rate, s.act + ci * label_rate * tracks, tracks, thresholds[k * n_classes + cls],
                                    label_rate, doa_threshold, margin, class_counters + o * N_CLASS_COUNTERS, class_de + o, status + o);
        }
        __syncthreads();                                                       // the entries are rewritten by the next group
    }
}

// the records of one file added up, a thread per output element ([K][n_classes][5] counters, then [K][n_classes] shares of
// total_DE): every thread walks the file's segments in segment order and adds the entries of status 0, so each sum -- the float64
// ones too -- is ONE running sum in that order and depends on that file's records alone
__global__ __launch_bounds__(SWEEP_THREADS) void seld_sweep_file_sum_kernel(const int *__restrict__ class_counters,
                                                                            const double *__restrict__ class_de, const int *__restrict__ status,
                                                                            int n_seg, int kc, int64_t *__restrict__ file_counters,
                                                                            double *__restrict__ file_de)
{
    const int j = blockIdx.x * SWEEP_THREADS + threadIdx.x, n_cnt = kc * N_CLASS_COUNTERS;
    const size_t file = blockIdx.y, first = file * (size_t)n_seg;
    if (j < n_cnt) {
        const int e = j / N_CLASS_COUNTERS;
        int64_t acc = 0;
        for (int seg = 0; seg < n_seg; seg++)
            if (status[(first + seg) * kc + e] == SCORED) acc += class_counters[(first + seg) * n_cnt + j];
        file_counters[file * n_cnt + j] = acc;
    } else if (j < n_cnt + kc) {
        const int e = j - n_cnt;
        double acc = 0.0;
        for (int seg = 0; seg < n_seg; seg++)
            if (status[(first + seg) * kc + e] == SCORED) acc += class_de[(first + seg) * kc + e];
        file_de[file * kc + e] = acc;
    }
}

int sfail(const char *msg)
{
    salsa_set_last_error_(msg);
    return -1;
}

} // namespace

extern "C" int salsa_nn_seld_sweep(const float *act, const float *xyz, int n_files, int n_in_frames, int n_frames, int n_classes, int multi,
                                   double cos_unify, const float *thresholds, int K, const int16_t *gt_rows, const int *gt_counts,
                                   int gt_capacity, int label_rate, double doa_threshold, double margin, int *class_counters, double *class_de,
                                   int *status, int64_t *file_counters, double *file_de, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!act || !xyz || !thresholds || !gt_rows || !gt_counts || !class_counters || !class_de || !status)
        return sfail("salsa_nn_seld_sweep: NULL input, threshold table or record output");
    if ((file_counters == nullptr) != (file_de == nullptr)) return sfail("salsa_nn_seld_sweep: file_counters and file_de come together");
    if (((uintptr_t)act & 3) || ((uintptr_t)xyz & 3) || ((uintptr_t)thresholds & 3) || ((uintptr_t)gt_counts & 3) || ((uintptr_t)class_counters & 3) ||
        ((uintptr_t)status & 3) || ((uintptr_t)gt_rows & 7) || ((uintptr_t)class_de & 7) || ((uintptr_t)file_counters & 7) || ((uintptr_t)file_de & 7))
        return sfail("salsa_nn_seld_sweep: a misaligned pointer (rows and 8-byte values: 8 bytes)");
    if (n_files < 1 || n_files > 65535 || n_frames < 1 || n_frames > 32767 || n_in_frames < n_frames || n_in_frames > 32767 || gt_capacity < 1)
        return sfail("salsa_nn_seld_sweep: n_files outside 1 .. 65535, n_frames outside 1 .. 32767, n_in_frames < n_frames or gt_capacity < 1");
    if (label_rate < 1 || label_rate > MAX_RATE || n_classes < 1 || n_classes > MAX_CLASSES)
        return sfail("salsa_nn_seld_sweep: n_classes or label_rate outside 1 .. 32");
    if (K < 1 || K > seld_sweep::MAX_K) return sfail("salsa_nn_seld_sweep: K outside 1 .. 64");
    if (multi != 0 && multi != 1) return sfail("salsa_nn_seld_sweep: multi is 0 or 1");
    if (multi && !(cos_unify >= -1.0 && cos_unify <= 1.0)) return sfail("salsa_nn_seld_sweep: cos_unify is NaN or outside [-1, 1]");
    if (!(doa_threshold == doa_threshold) || !(margin >= 0.0) || margin == INFINITY)
        return sfail("salsa_nn_seld_sweep: a NaN doa_threshold, or a margin that is negative, NaN or infinite");
    const int n_seg = n_segments(n_frames, label_rate), kc = K * n_classes;
    hipLaunchKernelGGL(seld_sweep_kernel, dim3((unsigned)n_seg, (unsigned)n_files), dim3(SWEEP_THREADS), 0, (hipStream_t)hip_stream, act, xyz,
                       n_in_frames, n_frames, n_classes, multi, cos_unify, thresholds, K, (const DcaseRow *)gt_rows, gt_counts, gt_capacity, n_seg,
                       label_rate, doa_threshold, margin, class_counters, class_de, status);
    if (hipGetLastError() != hipSuccess) {
        salsa_set_last_error_("salsa_nn_seld_sweep: launch failed");
        return -6;
    }
    if (file_counters) {
        const int n_out = kc * (N_CLASS_COUNTERS + 1);
        hipLaunchKernelGGL(seld_sweep_file_sum_kernel, dim3((unsigned)((n_out + SWEEP_THREADS - 1) / SWEEP_THREADS), (unsigned)n_files),
                           dim3(SWEEP_THREADS), 0, (hipStream_t)hip_stream, class_counters, class_de, status, n_seg, kc, file_counters, file_de);
        if (hipGetLastError() != hipSuccess) {
            salsa_set_last_error_("salsa_nn_seld_sweep: launch failed");
            return -6;
        }
    }
    return 0;
}
