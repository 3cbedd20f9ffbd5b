// seld_score.hip -- salsa_nn_seld_score, salsa_nn_seld_score2020 and salsa_nn_seld_score2022 (include/salsa_nn.h): DCASE rows against
// ground-truth rows, the SELD 2021 counters of crnn/metrics.py::SeldMetrics, the SELD 2020 counters of SeldMetrics2020 or the per-class
// SELD 2022 counters of SeldMetrics2022, per (file, segment), on the device.  The statements are seld_score.h's; this file bins the
// rows, the same way for all three metrics.
//
// One workgroup of 256 threads (4 waves) per (file, segment).  Each side's rows are binned by seld_rows.h's walk (shared with
// seld_sweep.hip): in tiles of 256 consecutive rows, one
// 8-byte load per row; the tile's rows of this segment are compacted in ARRIVAL order (one ballot per wave, the wave counts through
// LDS, as seld_decode.hip does), and a compacted row's slot in its (class, frame) cell is the cell's count so far plus the number
// of earlier rows of the tile in the same cell: the cells fill in arrival order with no atomics, so two runs are bit-identical.
// Then one pass with a thread per cell pairs the cells that hold both sides, a thread per class does the class bookkeeping, and
// thread 0 writes the record (2020: a thread per cell takes the cell's least total cost, a thread per class walks its frames in
// ascending order).  Everything is float64 (a few hundred distances per workgroup: the float64 rate is no concern here,
// the walk over the rows is the cost).  seld_score_sum_kernel adds the scored records up in record order in one workgroup.  The 2022
// metric is the 2021 cells, pairing and class bookkeeping with the class axis kept in the record (seld_score2022_kernel), and its
// sums are per FILE, in segment order (seld_score2022_file_sum_kernel).
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/salsa_nn.h"
#include "seld_rows.h"
#include "seld_score.h"

namespace {

using namespace seld_score;

using seld_rows::DcaseRow;

constexpr int SCORE_THREADS = seld_rows::BIN_THREADS;

struct ScoreLds {                                                             // 46 KB
    Cell cells[MAX_CELLS];
    int gfirst[MAX_CELLS];
    uint8_t gcnt[MAX_CELLS], pcnt[MAX_CELLS], matched[MAX_CELLS], cell_doubt[MAX_CELLS];
    seld_rows::BinScratch bin;
    ClassResult res[MAX_CLASSES];
};

// the rows of one side of one file into the segment's cells, in arrival order: seld_rows.h's rule (every thread calls it)
template <bool IS_GT>
__device__ void bin_rows(ScoreLds &s, const DcaseRow *__restrict__ rows, int count, int seg, int label_rate, int n_classes)
{
    seld_rows::bin_rows(s.bin, IS_GT ? s.gcnt : s.pcnt, rows, count, seg, label_rate, n_classes, [&s](int cell, int slot, int32_t doa, int row) {
        if (slot < MAX_DOAS) (IS_GT ? s.cells[cell].in.g : s.cells[cell].in.p)[slot] = doa;
        if (IS_GT && slot == 0) s.gfirst[cell] = row;
    });
}

// the segment's rows into its cells, the cells paired and every class booked into s.res[0 .. n_classes - 1], valid after the closing
// barrier.  V2020: the SELD 2020 statements on the same cells.  (uniform: every thread of the workgroup calls it)
template <bool V2020>
__device__ __forceinline__ void score_classes(ScoreLds &s, const DcaseRow *__restrict__ pred, int n_pred, const DcaseRow *__restrict__ gt,
                                              int n_gt, int seg, int label_rate, int n_classes, double threshold, double margin)
{
    const int tid = threadIdx.x, n_cells = n_classes * label_rate;
    for (int c = tid; c < n_cells; c += SCORE_THREADS) {
        s.gcnt[c] = s.pcnt[c] = s.matched[c] = s.cell_doubt[c] = 0;
        s.gfirst[c] = 0;
    }
    __syncthreads();
    bin_rows<true>(s, gt, n_gt, seg, label_rate, n_classes);
    bin_rows<false>(s, pred, n_pred, seg, label_rate, n_classes);
    for (int c = tid; c < n_cells; c += SCORE_THREADS) {
        const int ng = s.gcnt[c], np = s.pcnt[c];
        if (ng < 1 || np < 1 || ng > MAX_DOAS || np > MAX_DOAS) continue;     // (a cell of more than 4 refuses its class in score_class)
        int32_t g[MAX_DOAS], p[MAX_DOAS];
        for (int k = 0; k < MAX_DOAS; k++) {
            g[k] = s.cells[c].in.g[k];
            p[k] = s.cells[c].in.p[k];
        }
        if constexpr (V2020) {
            s.cells[c].cost[0] = cell_cost2020(g, ng, p, np);                 // (over the DOAs just read)
        } else {
            double cost[MAX_DOAS] = {0.0, 0.0, 0.0, 0.0};
            bool doubt;
            const unsigned m = pair_cell(g, ng, p, np, margin, cost, &doubt);
            for (int k = 0; k < MAX_DOAS; k++) s.cells[c].cost[k] = cost[k];  // (over the DOAs just read)
            s.matched[c] = (uint8_t)m;
            s.cell_doubt[c] = doubt ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid < n_classes) {
        const int at = tid * label_rate;
        if constexpr (V2020)
            score_class2020(s.cells + at, s.gcnt + at, s.pcnt + at, label_rate, threshold, margin, &s.res[tid]);
        else
            score_class(s.cells + at, s.gcnt + at, s.pcnt + at, s.matched + at, s.cell_doubt + at, s.gfirst + at, label_rate, threshold, margin,
                        &s.res[tid]);
    }
    __syncthreads();
}

template <bool V2020>
__global__ __launch_bounds__(SCORE_THREADS) void seld_score_kernel(const DcaseRow *__restrict__ pred, const int *__restrict__ pred_counts,
                                                                   int pred_capacity, const DcaseRow *__restrict__ gt,
                                                                   const int *__restrict__ gt_counts, int gt_capacity, int n_seg,
                                                                   int label_rate, int n_classes, double threshold, double margin,
                                                                   int *__restrict__ counters, double *__restrict__ total_de,
                                                                   int *__restrict__ status)
{
    __shared__ ScoreLds s;
    const int tid = threadIdx.x, seg = blockIdx.x;
    const size_t file = blockIdx.y, record = file * (size_t)n_seg + seg;
    const int n_pred = pred_counts[file], n_gt = gt_counts[file];
    if (n_pred < 0 || n_pred > pred_capacity || n_gt < 0 || n_gt > gt_capacity) {   // (uniform) a count its slab cannot hold: nothing is read
        if (tid < N_COUNTERS) counters[record * N_COUNTERS + tid] = 0;
        if (tid == 0) {
            total_de[record] = 0.0;
            status[record] = REFUSED;
        }
        return;
    }
    score_classes<V2020>(s, pred + file * (size_t)pred_capacity, n_pred, gt + file * (size_t)gt_capacity, n_gt, seg, label_rate, n_classes,
                         threshold, margin);
    if (tid == 0) {
        if constexpr (V2020) segment_record2020(s.res, n_classes, counters + record * N_COUNTERS, total_de + record, status + record);
        else segment_record(s.res, n_classes, counters + record * N_COUNTERS, total_de + record, status + record);
    }
}

// The class-wise SELD 2022 record of a (file, segment): the 2021 cells, pairing and class bookkeeping (score_classes<false>), then
// thread 0 forms S, D, I and the status, and a thread per class writes its five counters and its share of total_DE.
__global__ __launch_bounds__(SCORE_THREADS) void seld_score2022_kernel(const DcaseRow *__restrict__ pred, const int *__restrict__ pred_counts,
                                                                       int pred_capacity, const DcaseRow *__restrict__ gt,
                                                                       const int *__restrict__ gt_counts, int gt_capacity, int n_seg,
                                                                       int label_rate, int n_classes, double threshold, double margin,
                                                                       int *__restrict__ class_counters, double *__restrict__ class_de,
                                                                       int *__restrict__ sdi, int *__restrict__ status)
{
    __shared__ ScoreLds s;
    __shared__ int seg_status;
    const int tid = threadIdx.x, seg = blockIdx.x;
    const size_t file = blockIdx.y, record = file * (size_t)n_seg + seg;
    const int n_pred = pred_counts[file], n_gt = gt_counts[file];
    if (n_pred < 0 || n_pred > pred_capacity || n_gt < 0 || n_gt > gt_capacity) {   // (uniform) a count its slab cannot hold: nothing is read
        if (tid < n_classes * N_CLASS_COUNTERS) class_counters[record * n_classes * N_CLASS_COUNTERS + tid] = 0;   // (at most 160 of them)
        if (tid < n_classes) class_de[record * n_classes + tid] = 0.0;
        if (tid < 3) sdi[record * 3 + tid] = 0;
        if (tid == 0) status[record] = REFUSED;
        return;
    }
    score_classes<false>(s, pred + file * (size_t)pred_capacity, n_pred, gt + file * (size_t)gt_capacity, n_gt, seg, label_rate, n_classes,
                         threshold, margin);
    if (tid == 0) {
        int st;
        segment_sdi2022(s.res, n_classes, sdi + record * 3, &st);
        status[record] = st;
        seg_status = st;
    }
    __syncthreads();
    if (tid < n_classes)
        class_record2022(&s.res[tid], seg_status, class_counters + (record * n_classes + tid) * N_CLASS_COUNTERS, class_de + record * n_classes + tid);
}

// the scored records added up: the counters exactly (int64), total_DE as ONE running float64 sum in record order (thread 0 adds
// each tile of 256 values from LDS), so the sum does not depend on anything but the records
__global__ __launch_bounds__(SCORE_THREADS) void seld_score_sum_kernel(const int *__restrict__ counters, const double *__restrict__ total_de,
                                                                       const int *__restrict__ status, int64_t n_records,
                                                                       int64_t *__restrict__ sum_counters, double *__restrict__ sum_de)
{
    __shared__ double de[SCORE_THREADS];
    __shared__ int64_t part[SCORE_THREADS];
    const int tid = threadIdx.x;
    int64_t acc[N_COUNTERS];
    for (int k = 0; k < N_COUNTERS; k++) acc[k] = 0;
    double sum = 0.0;
    for (int64_t tile = 0; tile < n_records; tile += SCORE_THREADS) {
        const int64_t i = tile + tid;
        const bool scored = i < n_records && status[i] == SCORED;
        de[tid] = scored ? total_de[i] : 0.0;                                  // (x + 0.0 == x: the others do not change the sum)
        if (scored)
            for (int k = 0; k < N_COUNTERS; k++) acc[k] += counters[i * N_COUNTERS + k];
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < SCORE_THREADS; j++) sum += de[j];
        __syncthreads();
    }
    for (int k = 0; k < N_COUNTERS; k++) {
        part[tid] = acc[k];
        __syncthreads();
        for (int step = SCORE_THREADS / 2; step > 0; step >>= 1) {
            if (tid < step) part[tid] += part[tid + step];
            __syncthreads();
        }
        if (tid == 0) sum_counters[k] = part[0];
        __syncthreads();
    }
    if (tid == 0) *sum_de = sum;
}

// the 2022 records of one file added up, a workgroup per file and a thread per output element: the file's n_classes x 5 class
// counters, its n_classes shares of total_DE and S, D, I (at most 160 + 32 + 3 <= SCORE_THREADS elements).  Every thread walks the
// file's segments in segment order, so each sum -- the float64 ones too -- is ONE running sum in that order, with no atomics, and a
// file's sums depend on that file's records alone.
__global__ __launch_bounds__(SCORE_THREADS) void seld_score2022_file_sum_kernel(const int *__restrict__ class_counters,
                                                                                const double *__restrict__ class_de,
                                                                                const int *__restrict__ sdi, const int *__restrict__ status,
                                                                                int n_seg, int n_classes, int64_t *__restrict__ file_counters,
                                                                                double *__restrict__ file_de, int64_t *__restrict__ file_sdi)
{
    const int tid = threadIdx.x, n_cnt = n_classes * N_CLASS_COUNTERS;
    const size_t file = blockIdx.x, first = file * (size_t)n_seg;
    if (tid < n_cnt) {
        int64_t acc = 0;
        for (int seg = 0; seg < n_seg; seg++)
            if (status[first + seg] == SCORED) acc += class_counters[(first + seg) * n_cnt + tid];
        file_counters[file * n_cnt + tid] = acc;
    } else if (tid < n_cnt + n_classes) {
        const int c = tid - n_cnt;
        double acc = 0.0;
        for (int seg = 0; seg < n_seg; seg++)
            if (status[first + seg] == SCORED) acc += class_de[(first + seg) * n_classes + c];
        file_de[file * n_classes + c] = acc;
    } else if (tid < n_cnt + n_classes + 3) {
        const int k = tid - n_cnt - n_classes;
        int64_t acc = 0;
        for (int seg = 0; seg < n_seg; seg++)
            if (status[first + seg] == SCORED) acc += sdi[(first + seg) * 3 + k];
        file_sdi[file * 3 + k] = acc;
    }
}

__global__ void seld_distance_kernel(const int16_t *__restrict__ quads, int64_t n, double *__restrict__ out)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) out[i] = distance_deg(quads[4 * i], quads[4 * i + 1], quads[4 * i + 2], quads[4 * i + 3]);
}

// both exports: the argument checks, the per-segment launch of either metric and the shared sum
template <bool V2020>
int launch_score(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows, const int *gt_counts,
                 int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes, double doa_threshold, double margin,
                 int *counters, double *total_de, int *status, int64_t *sum_counters, double *sum_de, void *hip_stream)
{
    // everything is checked before the first device call (the CPU suite exercises these returns without a GPU)
    if (!pred_rows || !pred_counts || !gt_rows || !gt_counts || !counters || !total_de || !status) return -1;
    if (((uintptr_t)pred_rows & 7) || ((uintptr_t)gt_rows & 7) || ((uintptr_t)total_de & 7) || ((uintptr_t)sum_de & 7) || ((uintptr_t)sum_counters & 7)) return -1;
    if ((sum_counters == nullptr) != (sum_de == nullptr)) return -1;
    if (n_files < 1 || n_files > 65535 || n_frames < 1 || n_frames > 32767 || pred_capacity < 1 || gt_capacity < 1) return -1;
    if (label_rate < 1 || label_rate > MAX_RATE || n_classes < 1 || n_classes > MAX_CLASSES) return -1;
    if (!(doa_threshold == doa_threshold) || !(margin >= 0.0) || margin == INFINITY) return -1;
    const int n_seg = n_segments(n_frames, label_rate);
    hipLaunchKernelGGL(seld_score_kernel<V2020>, dim3((unsigned)n_seg, (unsigned)n_files), dim3(SCORE_THREADS), 0, (hipStream_t)hip_stream,
                       (const DcaseRow *)pred_rows, pred_counts, pred_capacity, (const DcaseRow *)gt_rows, gt_counts, gt_capacity, n_seg,
                       label_rate, n_classes, doa_threshold, margin, counters, total_de, status);
    if (hipGetLastError() != hipSuccess) return -6;
    if (sum_counters) {
        hipLaunchKernelGGL(seld_score_sum_kernel, dim3(1), dim3(SCORE_THREADS), 0, (hipStream_t)hip_stream, counters, total_de, status,
                           (int64_t)n_files * n_seg, sum_counters, sum_de);
        if (hipGetLastError() != hipSuccess) return -6;
    }
    return 0;
}

// the 2022 export: salsa_nn_seld_score's argument checks, the per-segment launch and the per-file sums
int launch_score2022(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows, const int *gt_counts,
                     int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes, double doa_threshold, double margin,
                     int *class_counters, double *class_de, int *sdi, int *status, int64_t *file_counters, double *file_de, int64_t *file_sdi,
                     void *hip_stream)
{
    if (!pred_rows || !pred_counts || !gt_rows || !gt_counts || !class_counters || !class_de || !sdi || !status) return -1;
    if (((uintptr_t)pred_rows & 7) || ((uintptr_t)gt_rows & 7) || ((uintptr_t)class_de & 7) || ((uintptr_t)file_de & 7) ||
        ((uintptr_t)file_counters & 7) || ((uintptr_t)file_sdi & 7))
        return -1;
    if ((file_counters == nullptr) != (file_de == nullptr) || (file_counters == nullptr) != (file_sdi == nullptr)) return -1;
    if (n_files < 1 || n_files > 65535 || n_frames < 1 || n_frames > 32767 || pred_capacity < 1 || gt_capacity < 1) return -1;
    if (label_rate < 1 || label_rate > MAX_RATE || n_classes < 1 || n_classes > MAX_CLASSES) return -1;
    if (!(doa_threshold == doa_threshold) || !(margin >= 0.0) || margin == INFINITY) return -1;
    static_assert(MAX_CLASSES * (N_CLASS_COUNTERS + 1) + 3 <= SCORE_THREADS, "a thread per element of a file's sums");
    const int n_seg = n_segments(n_frames, label_rate);
    hipLaunchKernelGGL(seld_score2022_kernel, dim3((unsigned)n_seg, (unsigned)n_files), dim3(SCORE_THREADS), 0, (hipStream_t)hip_stream,
                       (const DcaseRow *)pred_rows, pred_counts, pred_capacity, (const DcaseRow *)gt_rows, gt_counts, gt_capacity, n_seg,
                       label_rate, n_classes, doa_threshold, margin, class_counters, class_de, sdi, status);
    if (hipGetLastError() != hipSuccess) return -6;
    if (file_counters) {
        hipLaunchKernelGGL(seld_score2022_file_sum_kernel, dim3((unsigned)n_files), dim3(SCORE_THREADS), 0, (hipStream_t)hip_stream,
                           class_counters, class_de, sdi, status, n_seg, n_classes, file_counters, file_de, file_sdi);
        if (hipGetLastError() != hipSuccess) return -6;
    }
    return 0;
}

} // namespace

extern "C" int salsa_nn_seld_score(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows,
                                   const int *gt_counts, int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes,
                                   double doa_threshold, double margin, int *counters, double *total_de, int *status, int64_t *sum_counters,
                                   double *sum_de, void *hip_stream)
{
    return launch_score<false>(pred_rows, pred_counts, pred_capacity, gt_rows, gt_counts, gt_capacity, n_files, n_frames, label_rate, n_classes,
                               doa_threshold, margin, counters, total_de, status, sum_counters, sum_de, hip_stream);
}

extern "C" int salsa_nn_seld_score2020(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows,
                                       const int *gt_counts, int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes,
                                       double doa_threshold, double margin, int *counters, double *total_de, int *status,
                                       int64_t *sum_counters, double *sum_de, void *hip_stream)
{
    return launch_score<true>(pred_rows, pred_counts, pred_capacity, gt_rows, gt_counts, gt_capacity, n_files, n_frames, label_rate, n_classes,
                              doa_threshold, margin, counters, total_de, status, sum_counters, sum_de, hip_stream);
}

extern "C" int salsa_nn_seld_score2022(const int16_t *pred_rows, const int *pred_counts, int pred_capacity, const int16_t *gt_rows,
                                       const int *gt_counts, int gt_capacity, int n_files, int n_frames, int label_rate, int n_classes,
                                       double doa_threshold, double margin, int *class_counters, double *class_de, int *sdi, int *status,
                                       int64_t *file_counters, double *file_de, int64_t *file_sdi, void *hip_stream)
{
    return launch_score2022(pred_rows, pred_counts, pred_capacity, gt_rows, gt_counts, gt_capacity, n_files, n_frames, label_rate, n_classes,
                            doa_threshold, margin, class_counters, class_de, sdi, status, file_counters, file_de, file_sdi, hip_stream);
}

extern "C" int salsa_nn_seld_distance(const int16_t *quads, int64_t n, double *out, void *hip_stream)
{
    if (!quads || !out || n < 1 || n > ((int64_t)1 << 40) / 256 || ((uintptr_t)out & 7)) return -1;
    hipLaunchKernelGGL(seld_distance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, quads, n, out);
    return hipGetLastError() == hipSuccess ? 0 : -6;
}
