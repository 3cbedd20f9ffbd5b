// seld_rows.h -- the DCASE row as the device holds it, and the one rule by which a workgroup bins the rows of a (file, segment) into
// its (class, frame) cells: shared by seld_score.hip (both sides of salsa_nn_seld_score / _score2020 / _score2022) and seld_sweep.hip
// (the reference side of salsa_nn_seld_sweep); seld_decode.hip and multi_accdoa.hip write the same row.  Device code only.
//
// The rows are walked in tiles of 256 consecutive rows, one 8-byte load per row; the tile's rows of this segment are compacted in
// ARRIVAL order (one ballot per wave, the wave counts through LDS), and a compacted row's slot in its cell is the cell's count so far
// plus the number of earlier rows of the tile in the same cell: the cells fill in arrival order with no atomics, so two runs are
// bit-identical.  A cell's count saturates at seld_score::COUNT_SAT.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "seld_score.h"

namespace seld_rows {

struct alignas(8) DcaseRow { int16_t frame, cls, azimuth, elevation; };

constexpr int BIN_THREADS = 256, BIN_WAVES = BIN_THREADS / 64;

struct BinScratch {                                                           // LDS of one workgroup of BIN_THREADS threads
    int list_cell[BIN_THREADS];
    int32_t list_doa[BIN_THREADS];
    int list_row[BIN_THREADS];
    int wave_count[BIN_WAVES];
};

// rows [count] of one file into the cells of segment `seg`; cnt [n_classes * label_rate] the cells' counts so far (LDS, updated);
// store(cell, slot, packed DOA, row index) is called once per row of the segment, by one thread, with the row's arrival slot in its
// cell (slots of MAX_DOAS and beyond included: the caller drops them).  Every thread of the workgroup calls it (uniform trip counts:
// every thread reaches the barriers); it ends with a barrier.
template <class Store>
__device__ __forceinline__ void bin_rows(BinScratch &b, uint8_t *cnt, const DcaseRow *__restrict__ rows, int count, int seg, int label_rate,
                                         int n_classes, Store store)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int tile = 0; tile < count; tile += BIN_THREADS) {
        const int i = tile + tid;
        int cell = -1;
        DcaseRow r = {0, 0, 0, 0};
        if (i < count) {                                                       // count <= capacity: checked by the caller
            r = rows[i];
            cell = seld_score::cell_of(r.frame, r.cls, seg, label_rate, n_classes);
        }
        const unsigned long long mask = __ballot(cell >= 0);
        if (lane == 0) b.wave_count[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < BIN_WAVES; w++) {
            const int c = b.wave_count[w];
            if (w < wave) before += c;
            total += c;
        }
        if (cell >= 0) {
            const int at = before + __popcll(mask & ((1ull << lane) - 1ull));  // < BIN_THREADS: one entry per row of the tile at most
            b.list_cell[at] = cell;
            b.list_doa[at] = seld_score::pack_doa(r.azimuth, r.elevation);
            b.list_row[at] = i;
        }
        __syncthreads();
        int my_cell = -1, slot = 0;
        bool last = true;
        if (tid < total) {
            my_cell = b.list_cell[tid];
            slot = cnt[my_cell];
            for (int j = 0; j < tid; j++) slot += b.list_cell[j] == my_cell;
            for (int j = tid + 1; j < total; j++) last = last && b.list_cell[j] != my_cell;
        }
        __syncthreads();                                                       // every count of before this tile has been read
        if (my_cell >= 0) {
            store(my_cell, slot, b.list_doa[tid], b.list_row[tid]);
            if (last) cnt[my_cell] = (uint8_t)(slot + 1 < seld_score::COUNT_SAT ? slot + 1 : seld_score::COUNT_SAT);
        }
        __syncthreads();                                                       // the list and wave_count are rewritten by the next tile
    }
}

} // namespace seld_rows
