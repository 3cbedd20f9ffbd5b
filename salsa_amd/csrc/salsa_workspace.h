// salsa_workspace.h -- the ONE description of the caller-supplied workspace of salsa_extract_batch, salsa_eigvec_batch,
// salsa_eigvec_feature_batch and salsa_extract_multichannel: which regions it holds, in which order, how large each is and by how
// much a clip group is offset into each.  The three *_workspace_bytes queries return workspace_layout(...).total; the entry points
// and the schedules bind their pointers from the same struct (bind_workspace, salsa_internal.h).  Plain C++17 without HIP, so the
// host compiler builds it for tests/test_workspace_layout_cpu.py.
//
//   region        element                               per clip                     written by           read by
//   spill         float2 spectra [t][pair][bin] x 2     T * nch * nd float2          K1 (or relayout)     K2, K3, gate_doubt
//   gate masks    uint32 [32-bin group][t]              ceil(nd/32) * T words        K2                   K3 / fused / cov_eig_n
//   doubt mask    uint32 [32-bin group][t]              ceil(nd/32) * T words        K3                   gate_doubt
//   doubt flags   uint32, one per clip                  1 word (a launch group uses its first clip's)     K2 / memset, K3, gate_doubt
// followed by 256 spare bytes.  Every buffer is clip-major, so a group of clips [g0, g1) is a pointer offset of g0 strides.
#pragma once
#include <stddef.h>

namespace salsa_impl {

// ---- mask geometry (the kernels that use it: salsa_kernels.hip)
constexpr int TR_CH = 64;       // K2: frames per chunk
constexpr int TR_BINS = 32;     // K2: bins per mask word: valid32[b][32-bin group][t]

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Every kernel addresses a mask as [b][ceil(nd/32)][T] with no padding (K2 stores lane < frames-left, K3 reads and zeroes
// group < ceil(nd/32)), so T * ceil(nd/32) words per clip is what is touched.  Two SIZINGS of the region exist because the byte counts
// the queries return are part of the ABI's observable behaviour:
enum MaskSizing {
    MASK_CHUNKED, // the 4-channel entry points: whole 64-frame chunks and 64-bin groups (K2's chunk, one K3 wave's two words) -- never
                  // smaller than the tight size; gate masks AND doubt mask AND doubt flags
    MASK_TIGHT    // the N-microphone path: exactly T * ceil(nd/32) words -- what K2 and cov_eig_n_kernel index; gate masks only (no doubt mask)
};

struct WorkspaceLayout {
    size_t spill_off, spill_bytes; // byte offset and (256-aligned) byte size of each region, in this order
    size_t gate_off, gate_bytes;
    size_t doubt_off, doubt_bytes; // 0 bytes under MASK_TIGHT
    size_t flag_off, flag_bytes;   // 0 bytes under MASK_TIGHT
    size_t total;                  // what the caller must supply: the regions + 256 spare
    size_t spill_clip, mask_clip, flag_clip; // per-clip strides in bytes (mask_clip: gate masks and doubt mask alike)

    // byte offsets of the group that starts at clip g0; spill_group_bytes: the exact size of n_clips clips' spectra (what the fused
    // schedule may reuse for its float64 records)
    size_t spill_at(int g0) const { return spill_off + (size_t)g0 * spill_clip; }
    size_t gate_at(int g0) const { return gate_off + (size_t)g0 * mask_clip; }
    size_t doubt_at(int g0) const { return doubt_off + (size_t)g0 * mask_clip; }
    size_t flag_at(int g0) const { return flag_off + (size_t)g0 * flag_clip; }
    size_t spill_group_bytes(int n_clips) const { return (size_t)n_clips * spill_clip; }
};

// batch clips of T frames, nd DOA bins and nch (even) channels per clip
static inline WorkspaceLayout workspace_layout(int batch, size_t T, int nd, int nch, MaskSizing sizing)
{
    const size_t complex64 = 2 * sizeof(float); // one spectrum value (float2)
    WorkspaceLayout L;
    L.spill_clip = T * nch * nd * complex64;
    L.mask_clip = (size_t)((nd + TR_BINS - 1) / TR_BINS) * T * sizeof(unsigned);
    L.flag_clip = sizeof(unsigned);
    const bool chunked = sizing == MASK_CHUNKED;
    const size_t mask = chunked ? align256((size_t)batch * ((T + TR_CH - 1) / TR_CH) * ((nd + 63) / 64) * TR_CH * 2 * sizeof(unsigned))
                                : align256((size_t)batch * L.mask_clip);
    L.spill_off = 0;
    L.spill_bytes = align256((size_t)batch * L.spill_clip);
    L.gate_off = L.spill_off + L.spill_bytes;
    L.gate_bytes = mask;
    L.doubt_off = L.gate_off + L.gate_bytes;
    L.doubt_bytes = chunked ? mask : 0;
    L.flag_off = L.doubt_off + L.doubt_bytes;
    L.flag_bytes = chunked ? align256((size_t)batch * L.flag_clip) : 0;
    L.total = L.flag_off + L.flag_bytes + 256;
    return L;
}

} // namespace salsa_impl
