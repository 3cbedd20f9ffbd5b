// baseline_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the baseline SELD features (dataset/feature_extraction.py of the
// reference: log-mel / log-linear spectrograms + intensity vector or GCC-PHAT) and their C ABI (include/salsa_baseline.h).
//
// None of these features has a time recurrence: every output frame depends on its own STFT frame(s) only.  So each feature
// family is ONE kernel, one workgroup per (frame, clip), everything on chip:
//   1. the n_fft-point STFT of the 4 channels as two packed complex FFTs z = w * (y_a + i y_b) in float64 (Stockham
//      radix-4 passes, a final radix-2 pass for 512, through LDS), unpacked and rounded to complex64 like librosa.stft;
//   2. the 4 log rows: 10*log10(max(1e-10, sum_k W[f][k] |X_c[k]|^2)) in float32, W = the lin types' compression matrix or
//      melW, applied sparsely (each row's contiguous non-zero bin range and its weights);
//   3a. IV types: Re(conj(X_0) X_j) / (||IV|| + 1e-8) per bin in float32, projected through the same W / melW;
//   3b. GCC types: the 2*n_fft-point STFT (float64 -> complex64), the 6 cross spectra X_m conj(X_n) phase-normalised (R == 0:
//      phasor 1), and the inverse real FFTs of the 6 pairs as 3 packed complex FFTs in float32 (inputs are unit phasors,
//      outputs are bounded by 1); only the kept lags are written.
// The audio is read once per frame from HBM (the overlap of neighbouring frames is served by L2) and every output row is
// written once.  No workspace, no allocation, no synchronisation in the extract call: hipGraph-capturable.
//
// Arithmetic follows the reference (see DESIGN.md "Baseline features"): STFTs evaluated in float64 and stored as complex64;
// log rows and IV in float32 with the roundings of numpy's complex64 arithmetic written out (no FMA contraction); the lin
// GCC forms R in complex64, the mel GCC in complex128 (the reference's float64 freq_filter promotes it; the filter itself is
// positive and leaves angle(R) unchanged, so it is not applied).
#include "build_guard.h"
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../include/salsa_hip.h"
#include "../../include/salsa_baseline.h"
#include "salsa_math.h"
#include "salsa_internal.h" // salsa_set_last_error_: the message salsa_last_error() returns (salsa_plan.hip)

using salsa::cplx;

namespace {

int bfail(int code, const char *msg)
{
    salsa_set_last_error_(msg);
    return code;
}

constexpr int BL_NT = 256; // threads per workgroup (4 waves)
enum { KIND_SPEC = 0, KIND_IV = 1, KIND_GCC = 2 };

struct BParams {
    int T, hop, F, C;
    int lagh;                           // GCC: ceil(F / 2) lags taken from the end of cc (cc[-F//2:] in Python's floor division)
    int gcc_f64;                        // mel GCC: cross spectra in float64 (the reference's complex128 chain)
    const int *band_lo, *band_hi, *band_off; // row f reads bins [lo, hi) with weights wts[off ...]
    const float *wts;
    const double *win1, *win2;          // periodic Hann of win_len centred in n_fft / 2 n_fft, pre-scaled by the unpack's 1/2 (exact)
    const cplx<double> *tw1, *tw2;      // exp(-2 pi i m / n), m < n, for n = n_fft and 2 n_fft
};

// One Stockham pass of NTR transforms of N points in z[NTR][N] (radix R, sub-transform length Ns -> R Ns), in place: every
// thread holds its butterflies in registers across the workgroup barrier between the gather and the scatter.
template <typename T, int N, int NTR, int R> __device__ __forceinline__ void fft_pass(cplx<T> *z, const cplx<double> *__restrict__ tw, int Ns)
{
    constexpr int NBF = NTR * (N / R);
    constexpr int PER = (NBF + BL_NT - 1) / BL_NT;
    cplx<T> v[PER][R];
    int dst[PER];
    const int step = N / (Ns * R);
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int idx = threadIdx.x + BL_NT * i;
        dst[i] = -1;
        if (NBF % BL_NT == 0 || idx < NBF) {
            const int q = idx / (N / R), j = idx % (N / R), k = j & (Ns - 1);
            const cplx<T> *zq = z + q * N;
#pragma unroll
            for (int r = 0; r < R; r++) v[i][r] = zq[j + r * (N / R)];
#pragma unroll
            for (int r = 1; r < R; r++) {
                const cplx<double> w = tw[k * r * step];
                v[i][r] = salsa::cmul(v[i][r], cplx<T>{(T)w.re, (T)w.im});
            }
            salsa::dftR<R>(v[i]);
            dst[i] = q * N + (j - k) * R + k;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (dst[i] >= 0) {
#pragma unroll
            for (int r = 0; r < R; r++) z[dst[i] + r * Ns] = v[i][r];
        }
    __syncthreads();
}

// forward DFT (e^{-2 pi i nk/N}, natural order in and out) of NTR transforms; ends behind a workgroup barrier
template <typename T, int N, int NTR> __device__ __forceinline__ void block_fft(cplx<T> *z, const cplx<double> *__restrict__ tw)
{
    int Ns = 1;
    for (; Ns * 4 <= N; Ns *= 4) fft_pass<T, N, NTR, 4>(z, tw, Ns);
    if (Ns < N) fft_pass<T, N, NTR, 2>(z, tw, Ns);
}

// z[p][n] = w[n] (y_{2p}[s] + i y_{2p+1}[s]), s = t hop - N/2 + n reflected at both clip ends (np.pad(mode='reflect'): one fold
// suffices because the host refuses clips of <= N/2 samples); samples under a zero window are not read.  nz[c] (zero on entry)
// is set when channel c has a non-zero sample under the window: the packed transform leaves a digitally silent channel the
// round-off of its partner (~1e-16 |X_partner|) where the FFT of zeros is exactly 0, and angle(R) / IV / (||IV|| + 1e-8) of that
// round-off are not small, so unpack4 writes an exact 0 for a channel without a set flag.
template <int N> __device__ __forceinline__ void load_frame(cplx<double> *z, const float *__restrict__ clip, int Ns, int t, int hop,
                                                            const double *__restrict__ win, int *nz)
{
    for (int e = threadIdx.x; e < 2 * N; e += BL_NT) {
        const int p = e / N, n = e % N;
        const double w = win[n];
        cplx<double> v = {0.0, 0.0};
        if (w != 0.0) {
            int s = t * hop - N / 2 + n;
            s = s < 0 ? -s : s;
            s = s >= Ns ? 2 * (Ns - 1) - s : s;
            const float ya = clip[(size_t)(2 * p) * Ns + s], yb = clip[(size_t)(2 * p + 1) * Ns + s];
            if (ya != 0.f) nz[2 * p] = 1;     // (every writer stores the same value)
            if (yb != 0.f) nz[2 * p + 1] = 1;
            v = {w * (double)ya, w * (double)yb};
        }
        z[e] = v;
    }
}

// X[c][k] (complex64), k = 0 .. N/2, from the two packed transforms; exactly 0 for a channel that load_frame found silent
template <int N> __device__ __forceinline__ void unpack4(const cplx<double> *z, float2 *X, const int *nz)
{
    constexpr int NB = N / 2 + 1;
    for (int e = threadIdx.x; e < 2 * NB; e += BL_NT) {
        const int p = e / NB, k = e % NB;
        cplx<double> x0, x1;
        salsa::unpack_pair_prescaled(z[p * N + k], z[p * N + ((N - k) & (N - 1))], x0, x1);
        X[(2 * p) * NB + k] = nz[2 * p] ? make_float2((float)x0.re, (float)x0.im) : make_float2(0.f, 0.f);
        X[(2 * p + 1) * NB + k] = nz[2 * p + 1] ? make_float2((float)x1.re, (float)x1.im) : make_float2(0.f, 0.f);
    }
}

__device__ __forceinline__ float power32(const float2 x) // |x|^2 in float32: the rounded product, the second fused (as K1 does)
{
    const float t = x.x * x.x;
    return __builtin_fmaf(x.y, x.y, t);
}
// 10 log10(max(1e-10, p)); the clamp's own value is written as the constant -100, whatever the last bit of __log2f(1e-10f)
__device__ __forceinline__ float db10(float p) { return p > 1e-10f ? 3.01029995663981195f * __log2f(p) : -100.f; }

// rows [c0, c0 + nrows) of frame t: row c at feature f = g(sum_k W[f][k] * val(c, k))
template <typename V, typename G> __device__ __forceinline__ void project_rows(const BParams &kp, int nrows, int c0, float *o, int t, V val, G g)
{
    for (int e = threadIdx.x; e < nrows * kp.F; e += BL_NT) {
        const int c = e / kp.F, f = e % kp.F;
        const int lo = kp.band_lo[f], hi = kp.band_hi[f];
        const float *w = kp.wts + kp.band_off[f] - lo;
        float acc = 0.f;
        for (int k = lo; k < hi; k++) acc = __builtin_fmaf(w[k], val(c, k), acc);
        o[((size_t)(c0 + c) * kp.T + t) * kp.F + f] = g(acc);
    }
}

// phase-normalised cross spectrum X_m conj(X_n) (np.exp(1j * np.angle(R)); R == 0 -> 1)
__device__ __forceinline__ float2 phasor(const float2 xm, const float2 xn, const int f64)
{
#pragma clang fp contract(off)
    double re, im;
    if (f64) { // complex128 (mel GCC): the products of float32 values are exact in float64, one rounding per sum
        re = (double)xm.x * (double)xn.x + (double)xm.y * (double)xn.y;
        im = (double)xm.y * (double)xn.x - (double)xm.x * (double)xn.y;
    } else {   // complex64 (lin GCC): numpy's (a c - b (-d)), (a (-d) + b c) with every product and sum rounded to float32
        re = (double)(xm.x * xn.x + xm.y * xn.y);
        im = (double)(xm.y * xn.x - xm.x * xn.y);
    }
    if (re == 0.0 && im == 0.0) return make_float2(1.f, 0.f);
    const double s = 1.0 / sqrt(re * re + im * im);
    return make_float2((float)(re * s), (float)(im * s));
}

template <int N, int KIND>
__global__ __launch_bounds__(BL_NT) void baseline_kernel(const BParams kp, const float *__restrict__ audio, float *__restrict__ out, int Ns)
{
    constexpr int NB = N / 2 + 1;
    constexpr int N2 = 2 * N, NB2 = N + 1;
    __shared__ cplx<double> z[KIND == KIND_GCC ? 2 * N2 : 2 * N]; // the forward transforms; then the GCC's 3 float32 inverse transforms
    __shared__ float2 X[KIND == KIND_GCC ? 4 * NB2 : 4 * NB];     // complex64 spectra of the 4 channels
    __shared__ float ivn[KIND == KIND_IV ? 3 * NB : 1];           // IV / ||IV|| per bin
    __shared__ int nz[4];                                         // channel c has a non-zero sample in the current frame

    const int t = blockIdx.x, b = blockIdx.y;
    const float *clip = audio + (size_t)b * 4 * Ns;
    float *o = out + (size_t)b * kp.C * kp.T * kp.F;

    if (threadIdx.x < 4) nz[threadIdx.x] = 0;
    __syncthreads();
    load_frame<N>(z, clip, Ns, t, kp.hop, kp.win1, nz);
    __syncthreads();
    block_fft<double, N, 2>(z, kp.tw1);
    unpack4<N>(z, X, nz);
    __syncthreads();
    project_rows(kp, 4, 0, o, t, [&](int c, int k) { return power32(X[c * NB + k]); }, [](float a) { return db10(a); });

    if (KIND == KIND_IV) {
        for (int k = threadIdx.x; k < NB; k += BL_NT) {
#pragma clang fp contract(off)
            const float2 x0 = X[k];
            float iv[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float2 xj = X[(j + 1) * NB + k];
                iv[j] = x0.x * xj.x + x0.y * xj.y; // Re(conj(X0) Xj) in complex64
            }
            const float nrm = sqrtf(iv[0] * iv[0] + iv[1] * iv[1] + iv[2] * iv[2]) + 1e-8f;
#pragma unroll
            for (int j = 0; j < 3; j++) ivn[j * NB + k] = iv[j] / nrm;
        }
        __syncthreads();
        project_rows(kp, 3, 4, o, t, [&](int c, int k) { return ivn[c * NB + k]; }, [](float a) { return a; });
    }

    if (KIND == KIND_GCC) {
        if (threadIdx.x < 4) nz[threadIdx.x] = 0; // (unpack4's reads of the first frame's flags ended at the barrier behind it)
        __syncthreads(); // the log rows' reads of X are done
        load_frame<N2>(z, clip, Ns, t, kp.hop, kp.win2, nz);
        __syncthreads();
        block_fft<double, N2, 2>(z, kp.tw2);
        unpack4<N2>(z, X, nz);
        __syncthreads();
        // spectra of the 3 packed inverse transforms, conjugated (IDFT(S) = conj(DFT(conj(S)))): transform g carries pair 2g in
        // its real part and pair 2g+1 in its imaginary part, both Hermitian-extended; DC and Nyquist are real (np.fft.irfft drops
        // their imaginary parts)
        cplx<float> *zf = reinterpret_cast<cplx<float> *>(z);
        constexpr int H = N2 / 2;
        for (int e = threadIdx.x; e < 3 * (H + 1); e += BL_NT) {
            const int g = e / (H + 1), k = e % (H + 1);
            const int n0 = g == 0 ? 0 : g == 1 ? 0 : 1, m0 = g == 0 ? 1 : g == 1 ? 3 : 3;  // pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3):
            const int n1 = g == 0 ? 0 : g == 1 ? 1 : 2, m1 = g == 0 ? 2 : g == 1 ? 2 : 3;  // g = 0: 01 + 02, 1: 03 + 12, 2: 13 + 23
            float2 a = phasor(X[m0 * NB2 + k], X[n0 * NB2 + k], kp.gcc_f64);
            float2 c = phasor(X[m1 * NB2 + k], X[n1 * NB2 + k], kp.gcc_f64);
            if (k == 0 || k == H) a.y = c.y = 0.f;
            zf[g * N2 + k] = {a.x - c.y, -(a.y + c.x)};                      // conj(A + i C)
            if (k > 0 && k < H) zf[g * N2 + N2 - k] = {a.x + c.y, a.y - c.x}; // conj(conj(A) + i conj(C))
        }
        __syncthreads();
        block_fft<float, N2, 3>(zf, kp.tw2);
        const float inv_n = 1.f / (float)N2; // exact
        for (int e = threadIdx.x; e < 6 * kp.F; e += BL_NT) {
            const int pr = e / kp.F, l = e % kp.F;
            const int j = l < kp.lagh ? N2 - kp.lagh + l : l - kp.lagh; // cc[-L//2:] ++ cc[:L//2]
            const cplx<float> v = zf[(pr >> 1) * N2 + j];
            o[((size_t)(4 + pr) * kp.T + t) * kp.F + l] = ((pr & 1) ? -v.im : v.re) * inv_n;
        }
    }
}

template <int N, int KIND> void launch(const BParams &kp, const float *audio, float *out, int B, int Ns, hipStream_t s)
{
    hipLaunchKernelGGL((baseline_kernel<N, KIND>), dim3(kp.T, B), dim3(BL_NT), 0, s, kp, audio, out, Ns);
}

const double PI = 3.14159265358979323846;

bool is_lin(int type) { return type == SALSA_BASELINE_LINSPECIV || type == SALSA_BASELINE_LINSPECGCC; }
bool is_gcc(int type) { return type == SALSA_BASELINE_MELSPECGCC || type == SALSA_BASELINE_LINSPECGCC; }

} // namespace

struct salsa_baseline_plan {
    salsa_baseline_params p;
    int C, F, kind;
    BParams kp;
    void *dev_mem; // one allocation: tables of kp
};

extern "C" {

int salsa_baseline_mel_matrix(int fs, int n_fft, int n_mels, double fmin, double fmax, float *out)
{
#pragma clang fp contract(off)
    if (fs <= 0 || n_fft <= 0 || n_mels <= 0 || !out) return bfail(SALSA_EINVAL, "salsa_baseline_mel_matrix: bad argument");
    if (fmax <= 0) fmax = (double)fs / 2;
    const int nb = 1 + n_fft / 2;
    // librosa 0.8.0 filters.mel: fft_frequencies = linspace(0, sr/2, nb); mel_f = mel_frequencies(n_mels + 2, fmin, fmax)
    // (Slaney: linear below 1 kHz, log above); weights[i] = max(0, min(-ramps[i] / fdiff[i], ramps[i+2] / fdiff[i+1])) stored
    // to float32, then weights *= 2 / (mel_f[i+2] - mel_f[i]) in float64 rounded back to float32.  np.linspace: i * step + start,
    // the last point set to stop.
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp; };
    auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m; };
    std::vector<double> fftf(nb), melf(n_mels + 2);
    {
        const double stop = (double)fs / 2, step = stop / (nb - 1);
        for (int k = 0; k < nb; k++) fftf[k] = (double)k * step + 0.0;
        fftf[nb - 1] = stop;
    }
    {
        const double a = hz_to_mel(fmin), z = hz_to_mel(fmax), step = (z - a) / (n_mels + 1);
        for (int i = 0; i < n_mels + 2; i++) melf[i] = mel_to_hz(i == n_mels + 1 ? z : (double)i * step + a);
    }
    for (int i = 0; i < n_mels; i++) {
        const double d0 = melf[i + 1] - melf[i], d1 = melf[i + 2] - melf[i + 1];
        const double enorm = 2.0 / (melf[i + 2] - melf[i]);
        for (int k = 0; k < nb; k++) {
            const double lower = -(melf[i] - fftf[k]) / d0, upper = (melf[i + 2] - fftf[k]) / d1;
            const double mn = lower < upper ? lower : upper;
            const float w = (float)(mn > 0.0 ? mn : 0.0);
            out[(size_t)i * nb + k] = (float)((double)w * enorm);
        }
    }
    return SALSA_OK;
}

int salsa_baseline_output_shape(const salsa_baseline_plan *pl, int64_t n_samples, int *n_channels, int64_t *n_frames, int *n_freq)
{
    if (!pl || n_samples <= 0) return bfail(SALSA_EINVAL, "salsa_baseline_output_shape: bad argument");
    if (n_channels) *n_channels = pl->C;
    if (n_frames) *n_frames = 1 + n_samples / pl->p.hop_len;
    if (n_freq) *n_freq = pl->F;
    return SALSA_OK;
}

size_t salsa_baseline_workspace_bytes(const salsa_baseline_plan *, int, int64_t) { return 0; }

int salsa_baseline_plan_destroy(salsa_baseline_plan *pl)
{
    if (!pl) return SALSA_OK;
    if (pl->dev_mem) (void)hipFree(pl->dev_mem);
    delete pl;
    return SALSA_OK;
}

int salsa_baseline_plan_create(const salsa_baseline_params *params, salsa_baseline_plan **out_plan)
{
    if (!params || !out_plan) return bfail(SALSA_EINVAL, "salsa_baseline_plan_create: NULL argument");
    *out_plan = nullptr;
    salsa_baseline_params p = *params;
    if (p.feature_type < SALSA_BASELINE_MELSPEC || p.feature_type > SALSA_BASELINE_LINSPECGCC)
        return bfail(SALSA_EINVAL, "salsa_baseline_plan_create: unknown feature type");
    if (p.n_fft != 256 && p.n_fft != 512) return bfail(SALSA_ENFFT, "nfft is not 512 or 256");
    if (p.win_len <= 0) p.win_len = p.n_fft;
    if (p.win_len > p.n_fft) return bfail(SALSA_EINVAL, "Windown length is greater than nfft!");
    if (p.fs <= 0 || p.hop_len <= 0) return bfail(SALSA_EINVAL, "salsa_baseline_plan_create: fs and hop_len must be positive");
    const int n = p.n_fft, nb = n / 2 + 1, n2 = 2 * n;
    const bool lin = is_lin(p.feature_type), gcc = is_gcc(p.feature_type);
    int F;
    if (lin) {
        F = p.is_compressed_freq ? (n == 512 ? 200 : 100) : n / 2;
    } else {
        if (p.n_mels <= 0) return bfail(SALSA_EINVAL, "salsa_baseline_plan_create: n_mels must be positive");
        if (gcc && p.n_mels > n2) return bfail(SALSA_EINVAL, "salsa_baseline_plan_create: n_mels exceeds the GCC length 2 * n_fft");
        F = p.n_mels;
    }
    // projection rows: [lo, hi) and their weights
    std::vector<int> lo(F), hi(F), off(F);
    std::vector<float> wts;
    if (lin) {
        const int ident = p.is_compressed_freq ? (n == 512 ? 192 : 96) : n / 2;
        for (int i = 0; i < F; i++) {
            off[i] = (int)wts.size();
            if (i < ident) {
                lo[i] = i + 1, hi[i] = i + 2;
                wts.push_back(1.0f);
            } else {
                lo[i] = ident + 1 + (i - ident) * 8, hi[i] = lo[i] + (i < F - 1 ? 8 : 7);
                for (int k = lo[i]; k < hi[i]; k++) wts.push_back(0.125f);
            }
        }
    } else {
        std::vector<float> mel((size_t)F * nb);
        int rc = salsa_baseline_mel_matrix(p.fs, n, F, p.fmin, p.fmax, mel.data());
        if (rc) return rc;
        for (int i = 0; i < F; i++) {
            int a = 0, z = 0;
            for (int k = 0; k < nb; k++)
                if (mel[(size_t)i * nb + k] != 0.f) {
                    if (z == 0) a = k;
                    z = k + 1;
                }
            lo[i] = a, hi[i] = z, off[i] = (int)wts.size();
            for (int k = a; k < z; k++) wts.push_back(mel[(size_t)i * nb + k]);
        }
    }
    // windows (librosa: periodic Hann of win_len, zero-padded centred to the FFT size; x 1/2 for the packed unpack) and twiddles
    std::vector<double> win1(n, 0.0), win2(n2, 0.0);
    for (int k = 0; k < p.win_len; k++) {
        const double w = 0.5 * (0.5 - 0.5 * cos(2.0 * PI * k / p.win_len));
        win1[(n - p.win_len) / 2 + k] = w;
        win2[(n2 - p.win_len) / 2 + k] = w;
    }
    std::vector<cplx<double>> tw1(n), tw2(n2);
    for (int m = 0; m < n; m++) tw1[m] = {cos(-2.0 * PI * m / n), sin(-2.0 * PI * m / n)};
    for (int m = 0; m < n2; m++) tw2[m] = {cos(-2.0 * PI * m / n2), sin(-2.0 * PI * m / n2)};

    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_tw1 = 0, o_tw2 = o_tw1 + al(16 * tw1.size()), o_w1 = o_tw2 + al(16 * tw2.size()), o_w2 = o_w1 + al(8 * win1.size()),
                 o_lo = o_w2 + al(8 * win2.size()), o_hi = o_lo + al(4 * F), o_off = o_hi + al(4 * F), o_wt = o_off + al(4 * F),
                 total = o_wt + al(4 * (wts.size() + 1));
    std::vector<char> host(total, 0);
    memcpy(host.data() + o_tw1, tw1.data(), 16 * tw1.size());
    memcpy(host.data() + o_tw2, tw2.data(), 16 * tw2.size());
    memcpy(host.data() + o_w1, win1.data(), 8 * win1.size());
    memcpy(host.data() + o_w2, win2.data(), 8 * win2.size());
    memcpy(host.data() + o_lo, lo.data(), 4 * F);
    memcpy(host.data() + o_hi, hi.data(), 4 * F);
    memcpy(host.data() + o_off, off.data(), 4 * F);
    memcpy(host.data() + o_wt, wts.data(), 4 * wts.size());
    void *dev = nullptr;
    hipError_t e = hipMalloc(&dev, total);
    if (e == hipSuccess) e = hipMemcpy(dev, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (dev) (void)hipFree(dev);
        char msg[256];
        snprintf(msg, sizeof(msg), "salsa_baseline_plan_create: %s", hipGetErrorString(e));
        return bfail(SALSA_EHIP, msg);
    }
    char *d = (char *)dev;
    salsa_baseline_plan *pl = new salsa_baseline_plan();
    pl->p = p;
    pl->F = F;
    pl->kind = gcc ? KIND_GCC : (p.feature_type == SALSA_BASELINE_MELSPEC ? KIND_SPEC : KIND_IV);
    pl->C = gcc ? 10 : pl->kind == KIND_IV ? 7 : 4;
    pl->dev_mem = dev;
    BParams &kp = pl->kp;
    kp.hop = p.hop_len, kp.F = F, kp.C = pl->C, kp.T = 0;
    kp.lagh = (F + 1) / 2;
    kp.gcc_f64 = p.feature_type == SALSA_BASELINE_MELSPECGCC;
    kp.tw1 = (const cplx<double> *)(d + o_tw1), kp.tw2 = (const cplx<double> *)(d + o_tw2);
    kp.win1 = (const double *)(d + o_w1), kp.win2 = (const double *)(d + o_w2);
    kp.band_lo = (const int *)(d + o_lo), kp.band_hi = (const int *)(d + o_hi), kp.band_off = (const int *)(d + o_off);
    kp.wts = (const float *)(d + o_wt);
    *out_plan = pl;
    return SALSA_OK;
}

int salsa_baseline_extract_batch(salsa_baseline_plan *pl, const float *d_audio, int batch, int64_t n_samples, float *d_out,
                                 void *, size_t, void *hip_stream)
{
    if (!pl || !d_audio || !d_out || batch <= 0 || batch > 65535) return bfail(SALSA_EINVAL, "salsa_baseline_extract_batch: bad argument");
    const int n_fft = pl->p.n_fft, pad = pl->kind == KIND_GCC ? n_fft : n_fft / 2;
    if (n_samples <= pad) return bfail(SALSA_EINVAL, "salsa_baseline_extract_batch: clip too short for the reflect padding of the STFT");
    if (4 * n_samples >= (int64_t)1 << 31) return bfail(SALSA_EINVAL, "salsa_baseline_extract_batch: clip too long");
    BParams kp = pl->kp;
    kp.T = (int)(1 + n_samples / pl->p.hop_len);
    if ((int64_t)kp.C * kp.T * kp.F >= (int64_t)1 << 31) return bfail(SALSA_EINVAL, "salsa_baseline_extract_batch: clip too long");
    const int Ns = (int)n_samples;
    hipStream_t s = (hipStream_t)hip_stream;
    if (n_fft == 512) {
        if (pl->kind == KIND_SPEC) launch<512, KIND_SPEC>(kp, d_audio, d_out, batch, Ns, s);
        else if (pl->kind == KIND_IV) launch<512, KIND_IV>(kp, d_audio, d_out, batch, Ns, s);
        else launch<512, KIND_GCC>(kp, d_audio, d_out, batch, Ns, s);
    } else {
        if (pl->kind == KIND_SPEC) launch<256, KIND_SPEC>(kp, d_audio, d_out, batch, Ns, s);
        else if (pl->kind == KIND_IV) launch<256, KIND_IV>(kp, d_audio, d_out, batch, Ns, s);
        else launch<256, KIND_GCC>(kp, d_audio, d_out, batch, Ns, s);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char msg[256];
        snprintf(msg, sizeof(msg), "salsa_baseline_extract_batch: launch failed: %s", hipGetErrorString(e));
        return bfail(SALSA_EHIP, msg);
    }
    return SALSA_OK;
}

} // extern "C"
