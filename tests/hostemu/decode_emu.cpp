// tests/hostemu/decode_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/seld_decode.h (the per-element arithmetic of
// salsa_nn_seld_decode).  TEST INFRASTRUCTURE ONLY: tests/test_test_chunks_cpu.py builds it with g++ -ffp-contract=off and holds the
// chunk combination and the angle rounding to numpy where there is no GPU.  The product never loads it and has no CPU path.
#include "../../salsa_amd/csrc/seld_decode.h"
using namespace seld_decode;

extern "C" {

int emu_expected_chunks(int n_frames, int chunk_len, int chunk_hop) { return expected_chunks(n_frames, chunk_len, chunk_hop); }

float emu_combine_step(float old, float fresh, int i, int off, int overlap, int gmean) { return combine_step(old, fresh, i, off, overlap, gmean); }

// chunks [n_chunks][chunk_len][C] -> out [n_frames][C]
void emu_combine(const float *chunks, int n_chunks, int chunk_len, int chunk_hop, int n_frames, int C, int gmean, float *out)
{
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < C; c++) out[(long)f * C + c] = file_value(chunks, n_chunks, chunk_len, chunk_hop, n_frames, C, f, c, gmean);
}

// xyz [n][3] -> azimuth [n], elevation [n]
void emu_angles(const float *xyz, long n, int16_t *azimuth, int16_t *elevation)
{
    for (long i = 0; i < n; i++) xyz_to_angles(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], azimuth + i, elevation + i);
}

// one file, serially, what the kernel's workgroup does: rows [n_frames * nc][4]; returns the number of rows
int emu_decode(const float *sed, const float *xyz, int n_chunks, int chunk_len, int chunk_hop, int n_frames, int nc, float threshold,
               int gmean, int16_t *rows)
{
    int n = 0;
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < nc; c++) {
            if (!is_active(file_value(sed, n_chunks, chunk_len, chunk_hop, n_frames, nc, f, c, gmean), threshold)) continue;
            float v[3];
            for (int k = 0; k < 3; k++) v[k] = file_value(xyz, n_chunks, chunk_len, chunk_hop, n_frames, 3 * nc, f, k * nc + c, gmean);
            rows[4 * n] = (int16_t)f;
            rows[4 * n + 1] = (int16_t)c;
            xyz_to_angles(v[0], v[1], v[2], rows + 4 * n + 2, rows + 4 * n + 3);
            n++;
        }
    return n;
}
}
