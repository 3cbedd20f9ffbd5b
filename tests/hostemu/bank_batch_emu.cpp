// tests/hostemu/bank_batch_emu.cpp -- CPU unit-test harness for salsa_amd/csrc/bank_batch.h (the per-element arithmetic of
// salsa_bank_batch and of salsa_augment_batch / salsa_augment_gcc_batch).  TEST INFRASTRUCTURE ONLY: tests/test_bank_batch_cpu.py
// builds it with g++ -ffp-contract=off as a shared object and holds the loops below to the composed torch path where there is no GPU,
// and as a stand-alone program with -fsanitize=address,undefined, whose main() runs the edge cases on banks allocated at their exact
// size (a read one element outside the bank is a report).  The product never loads it and has no CPU path.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../salsa_amd/csrc/bank_batch.h"
using namespace bank_batch;

// the three launches of bank_batch.hip as loops: labels, min / max of every unaugmented chunk, gather
extern "C" int emu_bank_batch(const float *bank, int C, int64_t bank_frames, int F, const float *sed_all, const float *doa_all,
                              int64_t label_total, int nc, const int64_t *start, const int64_t *gt_start, int B, int T, int L, int recipe,
                              int n_zero, const int *par, const float *uval, float *x, float *sed, float *doa)
{
    const int64_t plane = (int64_t)T * F, chan = bank_frames * F;
    for (int b = 0; b < B; b++) {
        if (start[b] < 0 || start[b] > bank_frames - T) return -1;
        if (sed_all) {
            const int64_t g = gt_start[b];
            if (g < 0 || g > label_total - L) return -1;
            for (int i = 0; i < L * nc; i++) sed[(int64_t)b * L * nc + i] = sed_all[g * nc + i];
            for (int l = 0; l < L; l++)
                for (int col = 0; col < 3 * nc; col++) {
                    const float *row = doa_all + (g + l) * 3 * nc;
                    doa[((int64_t)b * L + l) * 3 * nc + col] =
                        recipe == RECIPE_NONE ? row[col] : swap_target(row, col, nc, recipe == RECIPE_FOA, par + b * NPAR);
                }
        }
        const float *src = bank + start[b] * F;
        float mm[2] = {INFINITY, -INFINITY};
        for (int c = 0; c < C; c++)
            for (int64_t i = 0; i < plane; i++) {
                const float v = src[c * chan + i];
                mm[0] = fminf(mm[0], v);
                mm[1] = fmaxf(mm[1], v);
            }
        for (int t = 0; t < T; t++)
            for (int f = 0; f < F; f++) {
                float *dst = x + (int64_t)b * C * plane + (int64_t)t * F + f;
                if (recipe == RECIPE_NONE)
                    for (int c = 0; c < C; c++) dst[c * plane] = src[c * chan + (int64_t)t * F + f];
                else if (recipe == RECIPE_GCC)
                    augment10(src, chan, dst, plane, t, f, F, par + b * NPAR, uval + b * 8, mm);
                else
                    augment7(src, chan, dst, plane, t, f, F, recipe == RECIPE_MIC, n_zero, par + b * NPAR, uval + b * 8, mm);
            }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the sanitizer program
namespace {

int failures = 0;
void expect(bool ok, const char *what)
{
    if (!ok) { failures++; fprintf(stderr, "FAILED: %s\n", what); }
}

struct Lcg { // fixed fill: the runs repeat
    uint64_t s;
    float next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)((s >> 40) / 16777216.0 * 2.0 - 1.0); }
};

// one run on heap blocks of the exact sizes: every batch entry of `starts`, all bit patterns of the recipe cycled through the batch
void run_case(int C, int64_t bank_frames, int F, int nc, int T, int up, int recipe, int n_zero, const std::vector<int64_t> &starts,
              int shift, bool rects)
{
    const int B = (int)starts.size(), L = T / up;
    const int64_t label_total = bank_frames / up;
    std::vector<float> bank(C * bank_frames * F), sed_all(label_total * nc), doa_all(label_total * 3 * nc);
    Lcg g{12345u + (uint64_t)F};
    for (auto &v : bank) v = g.next();
    for (auto &v : sed_all) v = g.next() > 0.5f ? 1.f : 0.f;
    for (auto &v : doa_all) v = g.next();
    std::vector<int64_t> gts(B);
    std::vector<int> par((size_t)B * NPAR, 0);
    std::vector<float> u((size_t)B * 8);
    for (int b = 0; b < B; b++) {
        gts[b] = starts[b] / up;
        int *p = par.data() + (size_t)b * NPAR;
        for (int k = 0; k < 4; k++) p[k] = (b >> k) & 1;
        p[4] = shift;
        p[5] = b & 1;
        if (rects) { // eight rectangles that overlap, touch all four edges and include a full-width stripe
            const int top[8] = {0, T - 5, 3, 0, T / 2, 7, T - 1, 2}, h[8] = {4, 5, T - 3, T, 3, 9, 1, 6};
            const int left[8] = {0, F - 7, 0, F - 1, 0, 5, 0, F / 2}, w[8] = {6, 7, 3, 1, F, 11, F, 9};
            for (int r = 0; r < 8; r++) { p[8 + r] = top[r]; p[16 + r] = h[r]; p[24 + r] = left[r]; p[32 + r] = w[r]; }
        }
        for (int r = 0; r < 8; r++) u[(size_t)b * 8 + r] = 0.125f * r + 0.01f;
    }
    std::vector<float> x((size_t)B * C * T * F), sed((size_t)B * L * nc), doa((size_t)B * L * 3 * nc);
    const int rc = emu_bank_batch(bank.data(), C, bank_frames, F, sed_all.data(), doa_all.data(), label_total, nc, starts.data(),
                                  gts.data(), B, T, L, recipe, n_zero, par.data(), u.data(), x.data(), sed.data(), doa.data());
    expect(rc == 0, "emu_bank_batch refused a valid case");
    // what can be said without a second implementation: labels and un-augmented samples are copies
    for (int b = 0; b < B; b++) {
        expect(!memcmp(sed.data() + (size_t)b * L * nc, sed_all.data() + gts[b] * nc, sizeof(float) * L * nc), "sed window");
        const int *p = par.data() + (size_t)b * NPAR;
        const bool plain = recipe == RECIPE_NONE || (!p[0] && !p[1] && !p[2] && !p[3] && !shift && !rects);
        if (plain) {
            expect(!memcmp(doa.data() + (size_t)b * L * 3 * nc, doa_all.data() + gts[b] * 3 * nc, sizeof(float) * L * 3 * nc), "doa window");
            for (int c = 0; c < C; c++)
                expect(!memcmp(x.data() + ((size_t)b * C + c) * T * F, bank.data() + (c * bank_frames + starts[b]) * F, sizeof(float) * T * F),
                       "x window");
        }
    }
}

} // namespace

int main()
{
    const int T = 16, up = 8;
    const int64_t frames = 48;
    for (int F : {8, 191, 200}) {
        // the chunk at frame 0, the chunk that ends on the bank's last frame, overlapping and duplicate windows
        const std::vector<int64_t> edge = {0, frames - T, 8, 16, 8, 0, frames - T, 24};
        std::vector<int64_t> many(33);
        for (int b = 0; b < 33; b++) many[b] = (b * 8) % (frames - T + 1) / 8 * 8;
        for (int shift : {0, 1, 9}) {
            if (shift >= F) continue;
            for (bool rects : {false, true}) {
                run_case(7, frames, F, 12, T, up, RECIPE_FOA, 0, many, shift, rects);   // 33 samples: all 16 FOA patterns, twice
                run_case(7, frames, F, 14, T, up, RECIPE_MIC, 3, many, shift, rects);
                run_case(10, frames, F, 12, T, up, RECIPE_GCC, 6, many, shift, rects);
                run_case(7, frames, F, 12, T, up, RECIPE_MIC, 3, edge, shift, rects);
            }
        }
        run_case(7, frames, F, 12, T, up, RECIPE_NONE, 0, edge, 0, false);
        run_case(10, frames, F, 14, T, up, RECIPE_NONE, 0, {frames - T}, 0, false);      // B = 1
        run_case(7, T, F, 12, T, up, RECIPE_MIC, 3, {0}, 9 < F ? 9 : 1, true);           // the bank IS the chunk
    }
    // refusals: a window before the bank, a window past its end
    {
        std::vector<float> bank(7 * 16 * 8, 0.f), x(7 * 16 * 8);
        int64_t s = -1;
        expect(emu_bank_batch(bank.data(), 7, 16, 8, nullptr, nullptr, 0, 12, &s, nullptr, 1, 16, 2, RECIPE_NONE, 0, nullptr, nullptr,
                              x.data(), nullptr, nullptr) == -1, "start -1 refused");
        s = 1;
        expect(emu_bank_batch(bank.data(), 7, 16, 8, nullptr, nullptr, 0, 12, &s, nullptr, 1, 16, 2, RECIPE_NONE, 0, nullptr, nullptr,
                              x.data(), nullptr, nullptr) == -1, "start past the end refused");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    puts("bank_batch_emu: all edge cases clean");
    return 0;
}
