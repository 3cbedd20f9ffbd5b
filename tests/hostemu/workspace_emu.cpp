// workspace_emu.cpp -- salsa_amd/csrc/salsa_workspace.h (plain C++, the layout of the extractor's workspace) behind a C surface
// for tests/test_workspace_layout_cpu.py, and -- with its own main -- a stand-alone program that writes every clip group's share of every
// region into a buffer of exactly `total` bytes, for AddressSanitizer / UBSan.
#include "../../salsa_amd/csrc/salsa_workspace.h"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace salsa_impl;

extern "C" {

// out: spill_off, spill_bytes, gate_off, gate_bytes, doubt_off, doubt_bytes, flag_off, flag_bytes, total, spill_clip, mask_clip, flag_clip
void emu_workspace_layout(int batch, int64_t T, int nd, int nch, int tight, uint64_t *out)
{
    const WorkspaceLayout L = workspace_layout(batch, (size_t)T, nd, nch, tight ? MASK_TIGHT : MASK_CHUNKED);
    const size_t v[12] = {L.spill_off, L.spill_bytes, L.gate_off, L.gate_bytes, L.doubt_off, L.doubt_bytes,
                          L.flag_off,  L.flag_bytes,  L.total,    L.spill_clip, L.mask_clip,  L.flag_clip};
    for (int i = 0; i < 12; i++) out[i] = v[i];
}

// out: byte offsets of the group that starts at clip g0 -- spill, gate masks, doubt mask, doubt flag -- and the bytes of n_clips clips' spectra
void emu_workspace_group(int batch, int64_t T, int nd, int nch, int tight, int g0, int n_clips, uint64_t *out)
{
    const WorkspaceLayout L = workspace_layout(batch, (size_t)T, nd, nch, tight ? MASK_TIGHT : MASK_CHUNKED);
    out[0] = L.spill_at(g0);
    out[1] = L.gate_at(g0);
    out[2] = L.doubt_at(g0);
    out[3] = L.flag_at(g0);
    out[4] = L.spill_group_bytes(n_clips);
}

} // extern "C"

// every group of a G-way split writes its clips' bytes of every region it is given, inside an allocation of exactly `total` bytes
static void walk(int batch, size_t T, int nd, int nch, MaskSizing sizing, int G)
{
    const WorkspaceLayout L = workspace_layout(batch, T, nd, nch, sizing);
    unsigned char *w = (unsigned char *)malloc(L.total);
    if (!w) abort();
    if (G > batch) G = batch;
    for (int g = 0; g < G; g++) {
        const int g0 = (int)((long)batch * g / G), g1 = (int)((long)batch * (g + 1) / G);
        memset(w + L.spill_at(g0), 1 + g, L.spill_group_bytes(g1 - g0));
        memset(w + L.gate_at(g0), 1 + g, (size_t)(g1 - g0) * L.mask_clip);
        if (sizing == MASK_CHUNKED) {
            memset(w + L.doubt_at(g0), 1 + g, (size_t)(g1 - g0) * L.mask_clip);
            memset(w + L.flag_at(g0), 1 + g, L.flag_clip);
        }
    }
    free(w);
}

int main()
{
    const int nds[] = {1, 33, 64, 65, 191}, Ts[] = {1, 63, 64, 65, 161}, batches[] = {1, 5}, groups[] = {1, 2, 3, 8};
    for (int nd : nds)
        for (int T : Ts)
            for (int batch : batches)
                for (int G : groups) {
                    walk(batch, (size_t)T, nd, 4, MASK_CHUNKED, G);
                    walk(batch, (size_t)T, nd, 6, MASK_TIGHT, G);
                    walk(batch, (size_t)T, nd, 16, MASK_TIGHT, G);
                }
    puts("all layouts clean");
    return 0;
}
