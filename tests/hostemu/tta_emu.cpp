// tests/hostemu/tta_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/tta.h (the per-element arithmetic of salsa_nn_tta_variant and
// salsa_nn_tta_merge).  TEST INFRASTRUCTURE ONLY: tests/test_tta_cpu.py builds it with g++ -ffp-contract=off as a shared object and
// holds the loops below -- the kernels' grids walked serially -- to the torch operators where there is no GPU.  The product never
// loads it and has no CPU path.
#include <stdint.h>
#include "../../salsa_amd/csrc/tta.h"
using namespace tta;

extern "C" int emu_n_variants(int kind) { return n_variants(kind); }
extern "C" void emu_variant_bits(int kind, int v, int *m) { variant_bits(kind, v, m); }

// tta_variant_kernel<W>: width 4 asks for what the launcher asks for before it picks W = 4 (returns -2 when the shape has no such path)
template <int W> static void variant_loop(const float *in, int64_t in_batch, int64_t in_chan, float *out, int B, int T, int F, int kind, int v)
{
    const int64_t plane = (int64_t)T * F;
    int m[4];
    variant_bits(kind, v, m);
    for (int b = 0; b < B; b++)
        for (int64_t e = 0; e < plane; e += W) {
            const float *src = in + b * in_batch;
            if (kind == KIND_GCC) {
                const int t = (int)(e / F), f = (int)(e - (int64_t)t * F);
                variant10<W>(src, in_chan, out + b * 10 * plane, plane, t, f, F, v);
            } else {
                variant7<W>(src, in_chan, out + b * 7 * plane, plane, e, kind == KIND_MIC, m);
            }
        }
}

extern "C" int emu_variant(const float *in, int64_t in_batch, int64_t in_chan, float *out, int B, int T, int F, int kind, int v, int width)
{
    const int V = n_variants(kind);
    if (!V || v < 0 || v >= V) return -1;
    const int64_t plane = (int64_t)T * F;
    if (width == 4) {
        if (plane % 4 || in_chan % 4 || in_batch % 4 || ((uintptr_t)in & 15) || ((uintptr_t)out & 15) || (kind == KIND_GCC && F % 4)) return -2;
        variant_loop<4>(in, in_batch, in_chan, out, B, T, F, kind, v);
    } else {
        variant_loop<1>(in, in_batch, in_chan, out, B, T, F, kind, v);
    }
    return 0;
}

// tta_merge_kernel: one (cell, class) after the other
extern "C" int emu_merge(const float *prob, const float *xyz, int n_models, const int *variant_ids, int n_var, int kind, int B, int L, int nc,
                         float *prob_out, float *xyz_out)
{
    const int V = n_variants(kind);
    if (!V || n_models < 1 || n_var < 1 || n_var > MAX_VARIANTS) return -1;
    ids_t ids = {};
    for (int i = 0; i < n_var; i++) {
        if (variant_ids[i] < 0 || variant_ids[i] >= V) return -1;
        ids.v[i] = variant_ids[i];
    }
    const int64_t cells = (int64_t)B * L;
    for (int64_t cell = 0; cell < cells; cell++)
        for (int k = 0; k < nc; k++) {
            float o[4];
            merge_one(prob, xyz, n_models, ids, n_var, kind, cells, nc, cell, k, o);
            prob_out[cell * nc + k] = o[0];
            xyz_out[cell * 3 * nc + k] = o[1];
            xyz_out[cell * 3 * nc + nc + k] = o[2];
            xyz_out[cell * 3 * nc + 2 * nc + k] = o[3];
        }
    return 0;
}
