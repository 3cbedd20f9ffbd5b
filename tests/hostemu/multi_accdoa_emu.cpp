// tests/hostemu/multi_accdoa_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/multi_accdoa.h (the per-item arithmetic of
// salsa_nn_adpit_loss and salsa_nn_seld_decode_multi).  TEST INFRASTRUCTURE ONLY: tests/test_multi_accdoa_cpu.py builds it with
// g++ -ffp-contract=off and holds every decision to numpy where there is no GPU.  The product never loads it and has no CPU path.
#include "../../salsa_amd/csrc/multi_accdoa.h"
using namespace multi_accdoa;

extern "C" {

int emu_source_of(int k, int cand, int n) { return source_of(k, cand, n); }

// doa, doa_gt [rows][9 C], sed_gt [rows][3 C] -> chosen [rows][C], item [rows][C] float64, g_doa [rows][9 C]; serially, item by item
void emu_adpit(const float *doa, const float *sed_gt, const float *doa_gt, long rows, int C, uint8_t *chosen, double *item, float *g_doa)
{
    const double denom = 9.0 * (double)(rows * C);
    for (long r = 0; r < rows; r++)
        for (int c = 0; c < C; c++) {
            float P[9], T[9], sv[3], g[9];
            for (int m = 0; m < 3; m++) {
                sv[m] = sed_gt[r * 3 * C + m * C + c];
                for (int a = 0; a < 3; a++) {
                    P[m * 3 + a] = doa[r * 9 * C + (3 * a + m) * C + c];
                    T[m * 3 + a] = doa_gt[r * 9 * C + (3 * a + m) * C + c];
                }
            }
            chosen[r * C + c] = (uint8_t)adpit_item(P, sv, T, denom, item + r * C + c, g);
            for (int m = 0; m < 3; m++)
                for (int a = 0; a < 3; a++) g_doa[r * 9 * C + (3 * a + m) * C + c] = g[m * 3 + a];
        }
}

// one file, serially, what the kernel's workgroup does: act [n_frames][3 C], xyz [n_frames][9 C] -> rows [3 n_frames C][4], and per
// cell n_out, flags [n_frames][C] and the emitted vectors out [n_frames][C][3][3]; returns the number of rows
int emu_decode_multi(const float *act, const float *xyz, int n_frames, int C, float threshold, double cos_unify, int16_t *rows,
                     int *n_out, int *flags, float *out)
{
    int n = 0;
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < C; c++) {
            float a[3], v[9], o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < 3; t++) {
                a[t] = act[(long)f * 3 * C + t * C + c];
                for (int k = 0; k < 3; k++) v[t * 3 + k] = xyz[(long)f * 9 * C + (3 * k + t) * C + c];
            }
            const long cell = (long)f * C + c;
            const int m = unify_cell(a, v, threshold, cos_unify, o, flags + cell);
            n_out[cell] = m;
            for (int i = 0; i < 9; i++) out[cell * 9 + i] = i < 3 * m ? o[i] : 0.f;
            for (int g = 0; g < m; g++) {
                rows[4 * n] = (int16_t)f;
                rows[4 * n + 1] = (int16_t)c;
                seld_decode::xyz_to_angles(o[g * 3], o[g * 3 + 1], o[g * 3 + 2], rows + 4 * n + 2, rows + 4 * n + 3);
                n++;
            }
        }
    return n;
}
}
