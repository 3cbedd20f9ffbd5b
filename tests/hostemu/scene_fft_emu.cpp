// scene_fft_emu.cpp -- the scene renderer's per-lane transform arithmetic (salsa_amd/csrc/scene_fft.h) run on the CPU: a loop over 64
// lanes stands for the wave, in the order of scene_render.hip's wave_fft / wave_real_spectrum and its inverse.  Checks the packed half
// spectrum against a float64 DFT, one overlap-save block against the direct convolution, and the round trip.  A test harness
// (tests/test_scenes_cpu.py builds and runs it), never a fallback of the product.
#include "scene_fft.h"
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace scene;
static cf tw[1024];
static void fft512_lanes(cf v[64][8], cf *z)
{
    for (int l = 0; l < 64; l++) { salsa::dft8(v[l]); }
    for (int l = 0; l < 64; l++) lane_store(v[l], z, l, 1);
    for (int p = 8; p <= 64; p *= 8) {
        for (int l = 0; l < 64; l++) { lane_load(v[l], z, l); lane_pass(v[l], tw, l, p); }
        if (p == 8) for (int l = 0; l < 64; l++) lane_store(v[l], z, l, p);
    }
}
static void forward(const float *x, cf *S)
{
    cf v[64][8], z[Z_LEN];
    for (int l = 0; l < 64; l++) for (int r = 0; r < 8; r++) { int t = l + 64 * r; v[l][r] = {x[2 * t], x[2 * t + 1]}; }
    fft512_lanes(v, z);
    for (int l = 0; l < 64; l++) for (int r = 0; r < 8; r++) z[zpad(l + 64 * r)] = v[l][r];
    for (int l = 0; l < 64; l++) for (int r = 0; r < 8; r++) { int k = l + 64 * r; S[k] = real_unpack(z[zpad(k)], z[zpad((512 - k) & 511)], k, tw); }
}
static void inverse(const cf *S, float *y)
{
    cf v[64][8], z[Z_LEN];
    for (int l = 0; l < 64; l++) for (int r = 0; r < 8; r++) { int k = l + 64 * r; v[l][r] = salsa::cconj(real_pack(S[k], S[(512 - k) & 511], k, tw)); }
    fft512_lanes(v, z);
    for (int l = 0; l < 64; l++) for (int r = 0; r < 8; r++) { int t = l + 64 * r; y[2 * t] = v[l][r].re * (1.f / 512); y[2 * t + 1] = -v[l][r].im * (1.f / 512); }
}
int main()
{
    for (int m = 0; m < 1024; m++) tw[m] = {(float)cos(-2 * M_PI * m / 1024), (float)sin(-2 * M_PI * m / 1024)};
    std::vector<float> x(1024), h(1024, 0.f), y(1024);
    for (auto &a : x) a = rand() / (float)RAND_MAX - 0.5f;
    for (int i = 0; i < 512; i++) h[i] = rand() / (float)RAND_MAX - 0.5f;
    cf X[512], H[512], Y[512];
    forward(x.data(), X);
    forward(h.data(), H);
    double e1 = 0;
    for (int k = 0; k <= 512; k++) {
        std::complex<double> s = 0;
        for (int n = 0; n < 1024; n++) s += (double)x[n] * std::polar(1.0, -2 * M_PI * k * n / 1024);
        double er = k == 0 ? fabs(s.real() - X[0].re) : k == 512 ? fabs(s.real() - X[0].im) : std::abs(s - std::complex<double>(X[k].re, X[k].im));
        if (er > e1) e1 = er;
    }
    printf("forward max err %.3g\n", e1);
    for (int k = 0; k < 512; k++) Y[k] = spec_mac(cf{0, 0}, H[k], X[k], k == 0);
    inverse(Y, y.data());
    double e2 = 0;
    for (int n = 512; n < 1024; n++) {
        double s = 0;
        for (int j = 0; j < 512; j++) s += (double)h[j] * x[n - j];
        if (fabs(s - y[n]) > e2) e2 = fabs(s - y[n]);
    }
    printf("overlap-save max err %.3g\n", e2);
    inverse(X, y.data());
    double e3 = 0;
    for (int n = 0; n < 1024; n++) if (fabs(x[n] - y[n]) > e3) e3 = fabs(x[n] - y[n]);
    printf("round trip max err %.3g\n", e3);
    return !(e1 < 1e-4 && e2 < 1e-4 && e3 < 1e-5);
}
