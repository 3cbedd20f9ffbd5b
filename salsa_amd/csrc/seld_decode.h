// seld_decode.h -- per-element arithmetic of salsa_nn_seld_decode (seld_decode.hip): where the test chunks of a file lie, the value
// of one (frame, column) of the combined file output, and the integer angles of one DCASE row.  Host + device inline functions
// with no memory traffic but the reads of the chunk values; the same header compiles with g++ (tests/hostemu/decode_emu.cpp), so
// the arithmetic is checked against numpy on the CPU.  That host build is a test harness, never a fallback of the product.
//
// Reference semantics (paths relative to the upstream repository):
//   models/interfaces.py:97-139   combine_chunks: chunk starts arange(0, n_frames - chunk_len + 1, hop) plus the leftover start
//                                 n_frames - chunk_len; chunk 0 is copied, of chunk i >= 1 the first (chunk_len - hop) frames become
//                                 (old + new) / 2 (gmean: sqrt(old * new)) and the rest are overwritten -- a RUNNING pairwise
//                                 average in chunk order (three chunks over one frame weigh 1/4, 1/4, 1/2), for the leftover chunk too
//   models/interfaces.py:232-256  xyz -> round(atan2 in degrees), azimuth 180 -> -180
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SELD_HD __host__ __device__ __forceinline__
#else
#define SELD_HD inline
#endif

namespace seld_decode {

// the number of chunks a file of n_frames label frames is cut into; one chunk that is at least as long as the file is the
// whole-file case (placed from frame 0 and trimmed)
SELD_HD int expected_chunks(int n_frames, int chunk_len, int chunk_hop)
{
    if (chunk_len >= n_frames) return 1;
    const int span = n_frames - chunk_len;
    return span / chunk_hop + 1 + (span % chunk_hop != 0 ? 1 : 0);
}

// one step of the walk: `fresh` is chunk i's value `off` frames into the chunk, `old` what the earlier chunks left
SELD_HD float combine_step(float old, float fresh, int i, int off, int overlap, int gmean)
{
#if defined(__HIPCC__) // (the g++ harness is built with -ffp-contract=off)
#pragma clang fp contract(off)
#endif
    if (i == 0 || off >= overlap) return fresh;
    return gmean ? sqrtf(old * fresh) : (old + fresh) / 2.0f;
}

// the combined file value of (frame, col) from one file's chunks [n_chunks][chunk_len][C]; n_chunks == expected_chunks(...) and
// chunk_hop <= chunk_len <= n_frames when there is more than one chunk (the launcher checks both), so every frame is covered and
// the first chunk over a frame always overwrites.  Only the chunks that hold the frame are visited, in chunk order.
SELD_HD float file_value(const float *chunks, int n_chunks, int chunk_len, int chunk_hop, int n_frames, int C, int frame, int col,
                         int gmean)
{
    if (n_chunks == 1) return chunks[(long)frame * C + col];
    const int n_regular = (n_frames - chunk_len) / chunk_hop + 1, overlap = chunk_len - chunk_hop;
    const int lo = frame < chunk_len ? 0 : (frame - chunk_len) / chunk_hop + 1;
    const int hi = frame / chunk_hop < n_regular - 1 ? frame / chunk_hop : n_regular - 1;
    float v = 0.0f;
    for (int i = lo; i <= hi; i++) {
        const int off = frame - i * chunk_hop;
        v = combine_step(v, chunks[((long)i * chunk_len + off) * C + col], i, off, overlap, gmean);
    }
    if (n_chunks > n_regular && frame >= n_frames - chunk_len) { // the leftover chunk, last in the walk
        const int off = frame - (n_frames - chunk_len);
        v = combine_step(v, chunks[((long)(n_chunks - 1) * chunk_len + off) * C + col], n_chunks - 1, off, overlap, gmean);
    }
    return v;
}

// NaN is inactive
SELD_HD bool is_active(float sed, float threshold) { return sed >= threshold; }

// integer degrees of one direction, in float64 (the float32 inputs are exact in it): round-half-even of atan2 * 180 / pi
SELD_HD void xyz_to_angles(float xf, float yf, float zf, int16_t *azimuth, int16_t *elevation)
{
#if defined(__HIPCC__) // (the g++ harness is built with -ffp-contract=off)
#pragma clang fp contract(off)
#endif
    const double x = xf, y = yf, z = zf, pi = 3.141592653589793;
    const double a = rint(atan2(y, x) * 180.0 / pi), e = rint(atan2(z, sqrt(x * x + y * y)) * 180.0 / pi);
    int azi = a == a ? (int)a : 0; // (a NaN direction has no angle: 0, not an undefined conversion)
    const int ele = e == e ? (int)e : 0;
    if (azi == 180) azi = -180;
    *azimuth = (int16_t)azi;
    *elevation = (int16_t)ele;
}

} // namespace seld_decode
