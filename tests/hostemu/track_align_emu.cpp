// tests/hostemu/track_align_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/track_align.h (the per-cell arithmetic of
// salsa_nn_tta_merge_multi and salsa_nn_chunk_merge_multi).  TEST INFRASTRUCTURE ONLY: tests/test_track_align_cpu.py builds it with
// g++ -ffp-contract=off as a shared object and holds the loops below -- the kernels' grids walked serially -- to the numpy restatement
// where there is no GPU.  The product never loads it and has no CPU path.
#include <stdint.h>
#include "../../salsa_amd/csrc/track_align.h"
using namespace track_align;

// n cells R, V [n][track][axis] -> out [n] candidates
extern "C" void emu_align_cells(const float *R, const float *V, int64_t n, int *out)
{
    for (int64_t i = 0; i < n; i++) out[i] = align_cell(R + i * 9, V + i * 9);
}

static void store_cell(float *act_row, float *xyz_row, int C, int c, const float *a, const float *v)
{
    for (int n = 0; n < 3; n++) {
        act_row[n * C + c] = a[n];
        for (int k = 0; k < 3; k++) xyz_row[(3 * k + n) * C + c] = v[n * 3 + k];
    }
}

// tta_merge_multi_kernel: one (cell, class) after the other
extern "C" int emu_merge(const float *xyz, int n_models, const int *variant_ids, int n_var, int kind, int B, int L, int C, float *xyz_out,
                         float *act_out, int *perm)
{
    const int V = tta::n_variants(kind);
    if (!V || n_models < 1 || n_var < 1 || n_var > tta::MAX_VARIANTS) return -1;
    tta::ids_t ids = {};
    for (int i = 0; i < n_var; i++) {
        if (variant_ids[i] < 0 || variant_ids[i] >= V) return -1;
        ids.v[i] = variant_ids[i];
    }
    const int64_t cells = (int64_t)B * L;
    for (int64_t cell = 0; cell < cells; cell++)
        for (int c = 0; c < C; c++) {
            float v[9], a[3];
            merge_cell(xyz, n_models, ids, n_var, kind, cells, C, cell, c, v, a, perm);
            store_cell(act_out + cell * 3 * C, xyz_out + cell * 9 * C, C, c, a, v);
        }
    return 0;
}

// chunk_merge_multi_kernel: one (file, frame, class) after the other
extern "C" int emu_chunk_merge(const float *act, const float *xyz, int n_files, int n_chunks, int chunk_len, int chunk_hop, int n_frames,
                               int C, float *file_act, float *file_xyz)
{
    if (n_chunks > 1 && (chunk_hop > chunk_len || chunk_len > n_frames)) return -1;
    if (n_chunks != seld_decode::expected_chunks(n_frames, chunk_len, chunk_hop)) return -1;
    const int64_t chunk_rows = (int64_t)n_chunks * chunk_len;
    for (int64_t file = 0; file < n_files; file++)
        for (int frame = 0; frame < n_frames; frame++)
            for (int c = 0; c < C; c++) {
                float v[9], a[3];
                file_cell(act + file * chunk_rows * 3 * C, xyz + file * chunk_rows * 9 * C, n_chunks, chunk_len, chunk_hop, n_frames, C,
                          frame, c, a, v);
                const int64_t row = file * n_frames + frame;
                store_cell(file_act + row * 3 * C, file_xyz + row * 9 * C, C, c, a, v);
            }
    return 0;
}
