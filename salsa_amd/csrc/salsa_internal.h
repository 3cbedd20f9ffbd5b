// salsa_internal.h -- what the translation units of the feature extractor share with each other, and nothing else:
//   salsa_kernels.hip   K1 stft_kernel, K2 tracker_kernel, K3 cov_eig_kernel (+ gate_doubt_kernel, flex_allpass_kernel) and their launchers
//   fused_kernel.hip    the opt-in fused STFT + covariance / eigen kernel (salsa_plan_set_fused)
//   multichannel.hip    the N-microphone contrib path (cov_eig_n_kernel) and the spectra relayout
//   feature_utils.hip   the plan-free entry points (scaler, normalise, resample, PCM, augmentation, ...)
//   salsa_plan.hip      host code only: the plan, the schedules of salsa_extract_batch, the one error message
//   salsa_workspace.h   (plain C++, no HIP) the layout of the caller's workspace: regions, sizes, per-clip strides, the mask geometry
// A unit's kernels stay in its own anonymous namespace; another unit reaches them through the launchers declared at the end of this
// file.  The library is built without -fvisibility=hidden, so everything that crosses a unit boundary is marked SALSA_LOCAL: the
// shared object exports the C ABI of include/*.h and nothing more.  baseline_kernels.hip, bank_batch.hip and tta.hip include this header
// for salsa_set_last_error_ alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/salsa_hip.h"
#include "salsa_math.h"
#include "salsa_workspace.h" // TR_CH, TR_BINS, align256, WorkspaceLayout

#define SALSA_LOCAL __attribute__((visibility("hidden")))

// the message salsa_last_error() returns: ONE thread_local buffer, defined in salsa_plan.hip; every unit's failures land in it
extern "C" SALSA_LOCAL void salsa_set_last_error_(const char *msg);

namespace salsa_impl {

static inline int fail(int code, const char *fmt, const char *a = "", long b = 0)
{
    char msg[512];
    snprintf(msg, sizeof(msg), fmt, a, b);
    salsa_set_last_error_(msg);
    return code;
}

static inline int hip_fail(const char *expr, hipError_t e)
{
    char msg[512];
    snprintf(msg, sizeof(msg), "%s failed: %s", expr, hipGetErrorString(e));
    salsa_set_last_error_(msg);
    return SALSA_EHIP;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return salsa_impl::hip_fail(#expr, e_);                             \
    } while (0)

struct KParams {
    int B;
    int N;    // samples per channel (host checks 4*N < 2^31)
    int T;    // frames (host checks 7*T*F < 2^31 and the per-clip spill < 2^31 elements)
    int hop;
    int lower, upper, nd; // DOA band [lower, upper), nd = upper - lower
    int cutoff;           // lite: spectrogram band [lower, cutoff)
    int F;                // feature bins per frame
    int OC;               // output channels (7, or 4 for logspec-only)
    int ident;            // identity rows of W (192 | 96 | n_fft/2)
    int spec_lo, spec_hi; // bins [spec_lo, spec_hi) map to spectrogram rows k - spec_lo (1 .. ident+1 for the dataset scripts)
    int flex;             // contrib/salsa_flexible.py semantics (SALSA_FLAG_FLEX): raw-|X0| tracker, gate without tracking, ...
    int compress;
    int layout;
    int feature;          // SALSA_FEATURE_* ; 3 = logspec only
    int format;
    int tracking;
    int n_hop;
    int pair_sel;         // K1: -1 = both channel pairs of every frame in one launch; 0 / 1 = only channels {0,1} / {2,3}
    int nch;              // audio channels per clip (even): 4, or 6 / 8 on the multichannel contrib surface; OC = 2*nch - 1
    double cond;
    double inv_cond;      // 1/cond (0 when cond == 0: unused, cond <= 1 short-circuits the gate)
    double delta;         // 2 pi fs / (n_fft * 343)
    double snr_ratio;     // indicator_sig = mag > snr_ratio * floor (1.5, :36; contrib: floor_mask_ratio)
    const float *sc_mean; // optional fused normalise-on-load of the spectrogram channels: [4][F] mean / std, or NULL
    const float *sc_std;
    unsigned long long *stats; // optional solver counters (salsa_plan_set_stats), or NULL
    int force_f64;             // SALSA_FLAG_FORCE_F64: the float64 instantiation of the covariance / eigen kernel
    unsigned *doubt32;         // [B][32-bin group][T] bit mask of the TF bins whose coherence test the quartic could not decide
                               // (salsa_math.h SALSA_GATE_DOUBT; decided by gate_doubt_kernel after the launch), or NULL (ungated plans)
    unsigned *doubt_flag;      // one word per launch group: non-zero once ANY bin was flagged (zeroed by the tracker launch before the
                               // covariance / eigen launch, or by a memset on the tracker-less gated path): gate_doubt_kernel reads it and exits
};

constexpr int FEATURE_LOGSPEC_ONLY = 3;

// ---- constants both sides of a launch need (the kernels that use them: salsa_kernels.hip; defaults as measured there)
// (TR_CH, TR_BINS -- K2's frames per chunk and bins per mask word -- are part of the workspace's layout: salsa_workspace.h)
#ifndef K3_FT_N
#define K3_FT_N 8 // measured 2/4/8/16/32/64: 8 is fastest (tiles in bursts do ~10x the work of quiet ones: small tiles balance)
#endif
constexpr int K3_FT = K3_FT_N; // frames per tile; divides TR_CH so a tile's gate words sit in one chunk
#ifndef K3_NT_N
#define K3_NT_N 128 // threads = bins per workgroup (a multiple of 64: every wave owns one 64-bin group of the tracker's masks).  Measured 256 / 128 / 64:
                    // cov_eig 0.365 / 0.340 / 0.348 ms, step 1.023 / 1.000 / 1.013 (profiles/r4_ab_notes.txt): the work list of a tile is ~1.5 x 256
                    // items, so with 256 threads half the waves sat out the second pass at the barrier; two waves share evenly
#endif
constexpr int K3_NT = K3_NT_N;
// K3: the packed-float32 pair solve (cov_eig_kernel PK; what fused_kernel runs)
#ifndef SALSA_PK
#define SALSA_PK 1
#endif
// The packed solve's gate certificate needs |q'(c)| * (error of c = mu1 / cond) well below SALSA_PK_GATE_TOL: both
// grow as cond -> 1 (c -> mu1, where q' = prod(mu1 - mu_i)), so plans with cond_num below 2 take the float64 instantiation
// (the dataset scripts use 5; the goldens 5 and 2).
#define SALSA_PK_COND_MIN 2.0

// ---- device helpers of K1 that fused_kernel.hip repeats (and db10: the decibel self-test of feature_utils.hip)
__device__ __forceinline__ int swz(int e) { return e ^ ((e >> 3) & 7); }

__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// |x|^2 of a complex64 spectrum value in float32, as ONE explicitly written FMA of an explicitly rounded product.  Written
// `x.x * x.x + x.y * x.y` the compiler is free to contract it either way round (or not at all), and did so differently in two
// unrolled instances of the STFT kernel once the code around it changed (session 3: the spectrogram of bins 128 - 191 moved by one
// ulp against the fused kernel's, which the bit-identity test of the two schedules caught).
__device__ __forceinline__ float power32(const float2 x)
{
    const float t = x.x * x.x;
    return __builtin_fmaf(x.y, x.y, t);
}
// max(a, b) as ONE v_max_f32: fmaxf() first canonicalises its operand (a second v_max_f32 v, v, v per value -- a quieting no-op for
// anything but a signalling NaN, which no arithmetic here produces); same result, NaN handling included (IEEE maxNum)
__device__ __forceinline__ float max_raw(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float db10(float p) { return 3.01029995663981195f * __log2f(max_raw(1e-10f, p)); } // 10*log10(max(1e-10,p))

// Addressing: a wave-uniform base pointer (SGPR pair) + a 32-bit unsigned BYTE offset per lane lets the compiler use the
// "saddr" form of global loads/stores; `ptr[int_index]` instead costs two or three 64-bit VALU instructions per access
// (sign extension, shift, 64-bit add), and K1 / K3 are VALU-issue bound.  The host checks that a clip's arrays stay
// below 4 GiB.
template <typename V> __device__ __forceinline__ void st_off(V *base, unsigned byte_off, const V v) { *(V *)((char *)base + byte_off) = v; }
template <typename V> __device__ __forceinline__ V ld_off(const V *base, unsigned byte_off) { return *(const V *)((const char *)base + byte_off); }

} // namespace salsa_impl

constexpr int SALSA_MAX_GROUPS = 16; // clip groups of the pipelined schedule (salsa_plan_set_pipeline)

struct salsa_plan {
    salsa_params p;
    int device;
    int lower, upper, cutoff, nd, F, ident;
    int spec_lo, spec_hi, flex;
    double delta, snr_ratio;
    double *d_window;     // the log-spectrogram window: win_len Hann centre-padded to n_fft (SALSA); n_fft Hann (SALSA-Lite / IPD, contrib)
    double *d_window_doa; // the DOA spectra's window, n_fft Hann: the same table as d_window unless a SALSA plan has win_len < n_fft
    salsa::cplx<double> *d_tw;
    const float *sc_mean, *sc_std; // caller-owned device arrays set by salsa_plan_set_scaler (or NULL)
    unsigned long long *stats;     // caller-owned device counters set by salsa_plan_set_stats (or NULL)
    int fused;                     // salsa_plan_set_fused: 0 = three kernels; 1 = STFT -> tracker -> fused STFT + covariance / eigen (stage a)
    int timing;
    int stop_after; // measurement only: 1 = issue the STFT launch alone, 2 = STFT + tracker, 0 = the whole path (salsa_plan_set_timing(plan, -1 | -2))
    int n_kernels;
    hipEvent_t ev0[SALSA_MAX_KERNELS], ev1[SALSA_MAX_KERNELS]; // start/stop of each launch (timing mode only)
    const char *names[SALSA_MAX_KERNELS];
    // clip-group pipeline (salsa_plan_set_pipeline): stream 0 runs the STFT kernels of all groups back to back; group g's
    // tracker and covariance/eigen kernels run on stream 1+g, so the latency-bound tracker of one group hides under the
    // STFT / eigen work of its neighbours.  With SALSA_PIPE_SPLIT_PAIRS the STFT of a group is two launches (channels 0/1,
    // then 2/3) and the tracker -- which only needs channel 0 -- starts after the first.  With SALSA_PIPE_GRAPH the whole
    // fork/join is captured ONCE per (buffers, sizes) into a hipGraph and replayed with a single hipGraphLaunch.
    int n_groups;
    int pipe_flags;
    hipStream_t streams[SALSA_MAX_GROUPS + 1];
    hipEvent_t ev_fork, ev_stft[SALSA_MAX_GROUPS], ev_stft2[SALSA_MAX_GROUPS], ev_join[SALSA_MAX_GROUPS + 1];
    hipStream_t cap_stream;
    hipGraphExec_t gexec;
    struct GraphKey { // what a captured graph is good for: compared and assigned as a whole
        const float *audio;
        float *out;
        void *ws;
        const float *sc_mean, *sc_std;
        int batch, n_groups, flags;
        int64_t n_samples;
        bool operator==(const GraphKey &o) const
        {
            return audio == o.audio && out == o.out && ws == o.ws && sc_mean == o.sc_mean && sc_std == o.sc_std && batch == o.batch &&
                   n_groups == o.n_groups && flags == o.flags && n_samples == o.n_samples;
        }
    } gkey;
};

namespace salsa_impl {

// the workspace regions of the clip group that starts at clip g0 (salsa_workspace.h; g0 = 0: the whole batch).  The doubt mask and its
// flag are bound only where the caller's plan gates (with_doubt): kp.doubt32 == NULL is how the kernels know an ungated plan.
static inline void bind_workspace(const WorkspaceLayout &L, void *base, int g0, bool with_doubt, float4 *&Xs, unsigned *&valid, KParams &kp)
{
    unsigned char *w = (unsigned char *)base;
    Xs = (float4 *)(w + L.spill_at(g0));
    valid = (unsigned *)(w + L.gate_at(g0));
    kp.doubt32 = with_doubt ? (unsigned *)(w + L.doubt_at(g0)) : nullptr;
    kp.doubt_flag = with_doubt ? (unsigned *)(w + L.flag_at(g0)) : nullptr; // one per launch group: its first clip's
}

// refusals the entry points that run K1 share, word for word
static inline int refuse_short_clip(const salsa_plan *pl, int64_t n_samples)
{
    if (n_samples <= pl->p.n_fft / 2) return fail(SALSA_EINVAL, "clip shorter than n_fft/2 samples cannot be reflect-padded%s");
    return SALSA_OK;
}
static inline int refuse_other_device(const salsa_plan *pl)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != pl->device)
        return fail(SALSA_EINVAL, "the plan's tables live on the device that was current at salsa_plan_create; make it current%s");
    return SALSA_OK;
}
static inline int refuse_workspace(const void *d_workspace, size_t workspace_bytes, size_t need)
{
    if (!d_workspace || workspace_bytes < need) return fail(SALSA_EWORKSPACE, "workspace too small%s (need %ld bytes)", "", (long)need);
    return SALSA_OK;
}

// salsa_plan.hip
SALSA_LOCAL KParams make_kparams(const salsa_plan *pl, int batch, int64_t n_samples);
// salsa_kernels.hip (launch_cov_eig: FEAT = true | false; launch_stft_multi: NPAIRS = 3 | 4 | 0 -- instantiated there)
SALSA_LOCAL int launch_stft(salsa_plan *pl, const KParams &kp, const double *win, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s);
SALSA_LOCAL int launch_k1(salsa_plan *pl, const KParams &kp, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s);
template <int NPAIRS>
SALSA_LOCAL int launch_stft_multi(salsa_plan *pl, const KParams &kp, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s);
SALSA_LOCAL void launch_tracker(const KParams &kp, hipStream_t s, const float4 *Xs, unsigned *valid32);
template <bool FEAT>
SALSA_LOCAL void launch_cov_eig(const KParams &kp, dim3 grid, hipStream_t s, const float4 *Xs, const unsigned *valid,
                                float *out_feat, double *out_eig, unsigned char *gate);
SALSA_LOCAL void launch_flex_allpass(const KParams &kp, hipStream_t s, float *out);
// fused_kernel.hip
SALSA_LOCAL bool fused_eligible(const salsa_plan *pl, const KParams &kp);
SALSA_LOCAL size_t fused_cold_bytes(const KParams &kp);
SALSA_LOCAL int launch_fused(salsa_plan *pl, const KParams &kp, const float *d_audio, float *d_out, const unsigned *valid, void *cold, hipStream_t s);
// multichannel.hip
SALSA_LOCAL void launch_relayout(const float4 *X, float4 *Xs, int B, int nb, int Tn, hipStream_t s);

} // namespace salsa_impl
