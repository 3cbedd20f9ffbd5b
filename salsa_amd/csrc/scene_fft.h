// scene_fft.h -- per-lane arithmetic of the scene renderer's transforms (scene_render.hip), host + device.
//
// A real FFT of 1024 points is a complex FFT of 512 on z[t] = x[2t] + i x[2t+1]: one wave, 8 points per lane, three radix-8 Stockham
// passes (salsa_math.h: dft8, stockham_*) through a padded LDS line of 512 complex numbers.  Everything here is what ONE lane does between
// two barriers; the kernel owns the barriers and the loads and stores of its data.  The same functions compile with g++, where a loop over
// the 64 lanes stands for the wave, so the addressing and the pack / unpack algebra are checked on the CPU against numpy before they
// ever run on a GPU.
//
// Spectrum layout ("packed half spectrum", 512 complex): S[0] = (X[0], X[512]) -- both real -- and S[k] = X[k] for k = 1 .. 511.
// The product of two such spectra is complex for k >= 1 and component-wise at k = 0.
// tw is the table W^m = exp(-2 pi i m / 1024), m = 0 .. 1023, rounded from float64.
#pragma once
#include "salsa_math.h"

namespace scene {

using salsa::cplx;
typedef cplx<float> cf;

constexpr int FFT_N = 512;                     // complex points = samples per partition
constexpr int FFT_R = 8;                       // radix: 64 lanes x 8 points
constexpr int FFT_LANES = FFT_N / FFT_R;
constexpr int Z_LEN = FFT_N + FFT_N / 8;       // a padded line: one slot more every 8, so that a pass's strided stores spread over the banks

SALSA_HD int zpad(int i) { return i + (i >> 3); }

SALSA_HD void lane_load(cf *v, const cf *z, int lane)
{
#pragma unroll
    for (int r = 0; r < FFT_R; r++) v[r] = z[zpad(salsa::stockham_in(lane, r, FFT_N, FFT_R))];
}

SALSA_HD void lane_store(const cf *v, cf *z, int lane, int p)
{
#pragma unroll
    for (int r = 0; r < FFT_R; r++) z[zpad(salsa::stockham_out(lane, r, p, FFT_R))] = v[r];
}

// one twiddled pass (p = 8 or 64) on the eight points a lane holds
SALSA_HD void lane_pass(cf *v, const cf *tw, int lane, int p)
{
    const int step = 2 * salsa::stockham_tw(lane, 1, p, FFT_N, FFT_R);     // W_512^m = W_1024^(2m); r * step <= 882
#pragma unroll
    for (int r = 1; r < FFT_R; r++) v[r] = salsa::cmul(v[r], tw[r * step]);
    salsa::dft8(v);
}

// X[k] of the real 1024-point transform from a = Z[k] and b = Z[(512 - k) mod 512]; k = 0 gives the packed pair (X[0], X[512])
SALSA_HD cf real_unpack(cf a, cf b, int k, const cf *tw)
{
    if (k == 0) return {a.re + a.im, a.re - a.im};
    const cf e = {0.5f * (a.re + b.re), 0.5f * (a.im - b.im)};
    const cf o = {0.5f * (a.im + b.im), 0.5f * (b.re - a.re)};
    return salsa::cadd(e, salsa::cmul(tw[k], o));
}

// the inverse of real_unpack: Z'[k] from y = S[k] and m = S[(512 - k) mod 512], so that the inverse 512-point transform of Z' is
// y[2t] + i y[2t+1] of the real signal whose packed half spectrum is S
SALSA_HD cf real_pack(cf y, cf m, int k, const cf *tw)
{
    if (k == 0) return {0.5f * (y.re + y.im), 0.5f * (y.re - y.im)};
    const cf e = {0.5f * (y.re + m.re), 0.5f * (y.im - m.im)};
    const cf d = {0.5f * (y.re - m.re), 0.5f * (y.im + m.im)};
    const cf o = salsa::cmulc(d, tw[k]);                                   // d conj(W^k)
    return {e.re - o.im, e.im + o.re};
}

// acc += h x for packed half spectra: complex for k >= 1, component-wise at k = 0.  Written as fused multiply-adds in one fixed
// order, so that equal operands give equal bits wherever this runs.
SALSA_HD cf spec_mac(cf acc, cf h, cf x, bool k0)
{
    if (k0) return {fmaf(h.re, x.re, acc.re), fmaf(h.im, x.im, acc.im)};
    return {fmaf(-h.im, x.im, fmaf(h.re, x.re, acc.re)), fmaf(h.im, x.re, fmaf(h.re, x.im, acc.im))};
}

} // namespace scene
