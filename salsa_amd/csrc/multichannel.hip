// multichannel.hip -- the N-microphone contrib path (salsa_extract_multichannel, 6 - 16 channels; gfx950): K1 over 3 / 4 / n channel
// pairs and K2 through the launchers of salsa_kernels.hip, then cov_eig_n_kernel here (an N x N Hermitian eigenproblem per gated TF
// bin).  Also relayout_kernel, which brings caller-supplied spectra into the spill's layout for salsa_eigvec_batch (launch_relayout).
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include "salsa_internal.h"

using salsa::cplx;
using namespace salsa_impl;

namespace {

// ------------------------------------------------------------------------------------------------------------ K3, N channels
// contrib/salsa_flexible.py takes ANY number of microphones (stacked_covmat_eigh :52-77: an N x N Hermitian eigenproblem per
// gated TF bin).  The 4 x 4 closed form of cov_eig_kernel (salsa_kernels.hip) does not generalise, so 5 - 8 microphones
// (padded to an even count NCH = 6 | 8 with a silent channel, which only adds a zero eigenvalue) take this kernel: one lane per (frame, bin), summed covariance of
// the 2*n_hop+1 frames in float64, cyclic complex Jacobi with the rotations accumulated (eigenvalues = the diagonal, eigen-
// vectors = the accumulated columns), gate "largest > second largest * ew_thresh" (:353), feature angle(conj(u_0) u_c) / f
// (:360-362).  A completeness path, not a tuned one: the 2 x NCH^2 float64 matrices spill to scratch.
// NCH > 0: compile-time size, fully unrolled (6 | 8).  NCH == 0: any even count up to HERMN_MAX = 16 read from kp.nch -- the same code
// with run-time loop bounds and dynamically indexed scratch arrays (9 - 16 microphones: slower still, and as rare).
// The solver itself (hermn, hermn_rotate, hermn_gate_eigvec) is in salsa_math.h, where the host emulation reaches it.
using salsa::hermn;
static_assert(salsa::HERMN_MAX == SALSA_MAX_MICS, "the run-time-sized solver holds SALSA_MAX_MICS channels");

template <int NCH>
__global__ __launch_bounds__(64) void cov_eig_n_kernel(const KParams kp, const float4 *__restrict__ Xs,
                                                       const unsigned *__restrict__ valid32, float *__restrict__ out)
{
    constexpr int S = hermn<NCH>::S;
    const int n = NCH > 0 ? NCH : kp.nch, NP = n / 2;
    const int t = blockIdx.x, b = blockIdx.y, Tn = kp.T;
    const int ng32 = (kp.nd + TR_BINS - 1) / TR_BINS;
    float *of = out + ((long)b * kp.OC + n) * Tn * kp.F + (long)t * kp.F; // first spatial plane, this frame's row
    const long plane = (long)Tn * kp.F;
    const float4 *xclip = Xs + (long)b * Tn * NP * kp.nd;
    for (int bin = threadIdx.x; bin < kp.F; bin += 64) {
        float e[S - 1];
#pragma unroll
        for (int c = 0; c < S - 1; c++) e[c] = 0.f;
        bool gated = bin < kp.nd;
        if (gated && kp.tracking) gated = (valid32[((long)b * ng32 + (bin >> 5)) * Tn + t] >> (bin & 31)) & 1u;
        if (gated) {
            hermn<NCH> A, V;
#pragma unroll
            for (int i = 0; i < n; i++)
#pragma unroll
                for (int j = 0; j < n; j++) {
                    A.ar[i][j] = A.ai[i][j] = 0.0;
                    V.ar[i][j] = i == j ? 1.0 : 0.0;
                    V.ai[i][j] = 0.0;
                }
            for (int k = -kp.n_hop; k <= kp.n_hop; k++) { // summed covariance, wrap on the time axis (:316-318, :347-349)
                int tt = t + k;
                while (tt < 0) tt += Tn;
                while (tt >= Tn) tt -= Tn;
                double xr[S], xi[S];
#pragma unroll
                for (int pr = 0; pr < NP; pr++) {
                    const float4 v = xclip[((long)tt * NP + pr) * kp.nd + bin];
                    xr[2 * pr] = v.x; xi[2 * pr] = v.y; xr[2 * pr + 1] = v.z; xi[2 * pr + 1] = v.w;
                }
#pragma unroll
                for (int i = 0; i < n; i++)
#pragma unroll
                    for (int j = 0; j < n; j++) { // x_i conj(x_j)
                        A.ar[i][j] += xr[i] * xr[j] + xi[i] * xi[j];
                        A.ai[i][j] += xi[i] * xr[j] - xr[i] * xi[j];
                    }
            }
            double ur[S], ui[S];
            int sweeps;
            const bool good = salsa::hermn_gate_eigvec<NCH>(A, V, n, kp.cond, ur, ui, sweeps);
            if (good) {
                const int kb = bin + kp.lower;
                const double den = (double)((float)(kb == 0 ? 1 : kb) * (float)kp.delta); // float32 norm_freq (:188-190)
#pragma unroll
                for (int c = 1; c < n; c++) { // angle(conj(u_0) u_c) / f   (:360-362)
                    const double wr = ur[0] * ur[c] + ui[0] * ui[c], wi = ur[0] * ui[c] - ui[0] * ur[c];
                    e[c - 1] = (float)(atan2(wi, wr) / den);
                }
            }
            if (!good && !kp.tracking) e[0] = __builtin_nanf(""); // marks "failed the test" for flex_allpass_kernel
        }
#pragma unroll
        for (int c = 0; c < n - 1; c++) of[c * plane + bin] = e[c];
    }
}

// reference layout (n_bins, n_frames, 4) complex64 -> internal Xs[b][t][pair][bin] float4
__global__ void relayout_kernel(const float4 *__restrict__ X, float4 *__restrict__ Xs, int B, int nb, int Tn)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)B * nb * Tn * 2;
    if (idx >= total) return;
    const int bin = (int)(idx % nb);
    long r = idx / nb;
    const int pr = (int)(r % 2);
    r /= 2;
    const int t = (int)(r % Tn);
    const int b = (int)(r / Tn);
    Xs[idx] = X[(((long)b * nb + bin) * Tn + t) * 2 + pr];
}

} // namespace

namespace salsa_impl {

void launch_relayout(const float4 *X, float4 *Xs, int B, int nb, int Tn, hipStream_t s)
{
    const long total = (long)B * nb * Tn * 2;
    hipLaunchKernelGGL(relayout_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, Xs, B, nb, Tn);
}

} // namespace salsa_impl

extern "C" {

size_t salsa_multichannel_workspace_bytes(const salsa_plan *pl, int n_channels, int batch, int64_t n_samples)
{
    if (!pl || batch <= 0 || n_samples <= 0 || n_channels < 4 || n_channels > SALSA_MAX_MICS || (n_channels & 1)) return 0;
    if (pl->p.feature_type != SALSA_FEATURE_SALSA) return 256;
    return workspace_layout(batch, (size_t)(1 + n_samples / pl->p.hop_len), pl->nd, n_channels, MASK_TIGHT).total;
}

int salsa_extract_multichannel(salsa_plan *pl, const float *d_audio, int n_channels, int batch, int64_t n_samples, float *d_out,
                               void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!pl || !d_audio || !d_out || batch <= 0 || n_samples <= 0) return fail(SALSA_EINVAL, "salsa_extract_multichannel: bad argument%s");
    if (!pl->flex || pl->p.audio_layout != SALSA_LAYOUT_PLANAR)
        return fail(SALSA_EINVAL, "salsa_extract_multichannel is the contrib (SALSA_FLAG_FLEX) surface, planar audio%s");
    if (n_channels < 6 || n_channels > SALSA_MAX_MICS || (n_channels & 1))
        return fail(SALSA_EINVAL, "salsa_extract_multichannel takes an even number of channels from 6 to 16 (pad an odd count with a silent channel; <= 4: salsa_extract_batch)%s");
    if (const int rc = refuse_short_clip(pl, n_samples)) return rc;
    const int64_t T64 = 1 + n_samples / pl->p.hop_len;
    const int OC = 2 * n_channels - 1;
    if (n_samples * 4 * n_channels >= INT32_MAX || T64 * OC * pl->F >= INT32_MAX / 2 || T64 * n_channels * (pl->nd > 0 ? pl->nd : 1) >= INT32_MAX / 16 ||
        T64 > 65535 * 16)
        return fail(SALSA_EINVAL, "clip too long for 32-bit per-clip indexing (split it)%s");
    if (const int rc = refuse_other_device(pl)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    KParams kp = make_kparams(pl, batch, n_samples);
    kp.nch = n_channels;
    kp.OC = OC;
    kp.sc_mean = kp.sc_std = nullptr;
    const bool full = pl->p.feature_type == SALSA_FEATURE_SALSA;
    float4 *Xs = nullptr;
    unsigned *valid = nullptr;
    if (full) { // (this path has no doubt mask: cov_eig_n_kernel decides its gate in float64)
        const WorkspaceLayout lay = workspace_layout(batch, (size_t)kp.T, kp.nd, n_channels, MASK_TIGHT);
        if (const int rc = refuse_workspace(d_workspace, workspace_bytes, lay.total)) return rc;
        bind_workspace(lay, d_workspace, 0, false, Xs, valid, kp);
    }
    int rc = n_channels == 6 ? launch_stft_multi<3>(pl, kp, d_audio, d_out, Xs, s)
           : n_channels == 8 ? launch_stft_multi<4>(pl, kp, d_audio, d_out, Xs, s)
                             : launch_stft_multi<0>(pl, kp, d_audio, d_out, Xs, s); // 10 - 16: channel count at run time
    if (rc || !full) return rc;
    if (kp.tracking && kp.nd > 0) {
        launch_tracker(kp, s, Xs, valid);
        HIP_TRY(hipGetLastError());
    }
    dim3 grid((unsigned)kp.T, (unsigned)kp.B);
    if (n_channels == 6) hipLaunchKernelGGL(cov_eig_n_kernel<6>, grid, dim3(64), 0, s, kp, Xs, valid, d_out);
    else if (n_channels == 8) hipLaunchKernelGGL(cov_eig_n_kernel<8>, grid, dim3(64), 0, s, kp, Xs, valid, d_out);
    else hipLaunchKernelGGL(cov_eig_n_kernel<0>, grid, dim3(64), 0, s, kp, Xs, valid, d_out);
    HIP_TRY(hipGetLastError());
    if (!kp.tracking && kp.nd > 0) {
        launch_flex_allpass(kp, s, d_out);
        HIP_TRY(hipGetLastError());
    }
    return SALSA_OK;
}

} // extern "C"
