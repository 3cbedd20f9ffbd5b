// salsa_kernels.hip -- the three production kernels of the SALSA / SALSA-Lite feature path for gfx950 (MI355X, CDNA4) and their
// launchers.  Written for wave64 / 160 KiB LDS / HBM3E; no CUDA or multi-backend paths.
//
//   K1 stft_kernel      one wave per packed 512-point complex FFT (two real channels), Stockham radix-8 through LDS;
//                       unpacks to the 4 channel spectra, writes the log-spectrogram channels 0-3 straight to the
//                       output and spills the DOA band of the spectra (float32-rounded, like the reference's
//                       complex64 STFT) to the workspace as Xs[b][t][channel pair][bin] (float4).
//                       SALSA-Lite / IPD is K1 alone (log-spectrogram + inter-channel phase fused into the unpack).
//   K2 tracker_kernel   one lane per (clip, bin): 3-frame RMS of channel 0 and the sequential noise-floor tracker
//                       in float64 -> valid32[b][32-bin group][t] (per-frame indicator mask of the group's bins).
//   K3 cov_eig_kernel   per tile of 8 frames x 128 bins the gated TF bins are compacted into an LDS work list (an item = two
//                       neighbouring frames of one bin, at least one gated in: their 7-frame windows share 6 frames);
//                       one lane per item: Hermitian covariances accumulated in registers, eigen-gate + principal
//                       eigenvector (salsa_math.h), FOA / MIC normalisation, writes channels 4-6 (zeros where gated).
//                       gate_doubt_kernel re-decides the bins K3 flags; flex_allpass_kernel is K3's epilogue on the contrib surface.
// The kernels sit in this unit's anonymous namespace.  The host side -- the plan and the schedules of salsa_extract_batch, in
// salsa_plan.hip, and the N-microphone path in multichannel.hip -- reaches them through the launchers at the end of the file
// (declared in salsa_internal.h): launch_stft / launch_k1 / launch_stft_multi, launch_tracker, launch_cov_eig, launch_flex_allpass.
//
// Arithmetic types follow the reference (see DESIGN.md "Precision"): STFT evaluated in float64 and rounded to
// float32, log-spectrogram in float32, tracker / covariance / eigen-solve in float64.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include "salsa_internal.h"
#include <type_traits>

using salsa::cplx;
using namespace salsa_impl;

namespace {

// ------------------------------------------------------------------------------------------------------------ K1
// STFT + log-spectrogram (+ spill of the DOA band, or the SALSA-Lite phase features).
//
// Work item of ONE WAVE = one packed N-point complex FFT z = w*(y_c0 + i*y_c1) of a channel pair of one frame:
// 64 lanes x R points, Stockham radix-R passes exchanged through a wave-private LDS buffer (no workgroup barrier:
// the LDS serves a wave's DS instructions in order, so a wave-level scheduling fence is all the passes need).
// LDS element e lives at slot e ^ ((e>>3)&7): with 16-byte complex-float64 elements this XOR swizzle makes every
// pass's stride-R scatter (ds_write_b128, 8-lane groups) AND the unit-stride gather (ds_read_b128, its odd 16-lane
// groups) bank-conflict free without padding.  After the last pass lane L holds Z[L + 64 r] in registers, which is
// exactly the ownership the unpack wants: X_c0[k], X_c1[k] need Z[k] and Z[N-k], and Z[N-k] of k = L + 64 r sits in
// register R-1-r of lane 64-L, so the mirror is fetched with cross-lane shuffles (R/2 complex values) instead of a
// third trip through LDS.  The spectra are rounded to float32 like the reference's complex64 STFT and used straight
// from registers: 10*log10 of the power into output channels c0, c1 and the DOA band of both channels as ONE float4
// per bin into the spill.  A wave walks K1_NF consecutive frames x 2 pairs (no software prefetch: the registers it would
// need cost a wave per SIMD, measured slower); the first twiddle of each pass lives in registers, the window in LDS.
//
// N = 1024 (SALSA-Lite / IPD only): 64 lanes x 16 points.  Rather than a 16 KB wave-private buffer and a radix-16 (or a fifth
// radix-4) pass, the wave runs the 512-point plan TWICE -- on the even and on the odd samples, through the same 8 KB buffer -- and
// joins the halves in registers with one decimation-in-time radix-2 step: Z[k] = E[k] + W_1024^k O[k], Z[k + 512] = E[k] - W_1024^k O[k].
// Lane L holds E[L + 64 r] and O[L + 64 r] after the sub-transforms, so the join needs no exchange and leaves Z[L + 64 r], r < 16, in
// the lane: the ownership the unpack wants.  W_1024^(L + 64 r) = W_1024^L (one register pair) times W_16^r (compile-time constants).
// Same LDS round trips per point as a 16 x 16 x 4 plan (two), and the LDS per workgroup stays that of the 512-point kernel plus
// the longer window table.
template <int N> struct fft_cfg {
    static constexpr int NSUB = (N == 1024) ? 2 : 1;             // sub-transforms per item (even / odd samples), joined in registers
    static constexpr int NS = N / NSUB;                          // length of one Stockham transform
    static constexpr int R = (NS == 512) ? 8 : 4;                // points per lane of one transform; 64 lanes per transform either way
    static constexpr int NP = (NS == 512) ? 2 : 3;               // twiddled passes (p = R, R^2, ...)
};

// Store policy (round 5, profiles/r5_ab_nt_stores.txt): the 16-byte write-once streams -- K1's spill (K1_SPILL_NT) and K3's rows of
// channels 4 - 6 (K3_OUT_NT) -- leave as NON-TEMPORAL stores (nothing re-reads them before they leave the L2, and the audio lines
// consecutive frames share stay cached longer); the 4-byte spectrogram rows stay PLAIN stores: the write-back L2 merges them into
// full lines, which nt stores forgo (all-nt was measured slower, 0.54 vs 0.49 ms).  The fused kernel's ring / row stores are plain.
// base + zero-extended lane offset + a COMPILE-TIME byte constant added after the extension: the constant lands in the load's
// immediate offset field (inside the 32-bit sum it cannot -- the unsigned addition may wrap as far as the compiler knows -- and
// costs a v_add_u32 per load)
template <typename V> __device__ __forceinline__ V ld_off_c(const V *base, unsigned byte_off, int const_bytes) { return *(const V *)((const char *)base + byte_off + const_bytes); }
// Production default since round 5 (0 = plain stores, for A/B): the spill's 16-byte stores as non-temporal stores ALONE (whole 1-KB
// wave stores that nothing re-reads before they leave the L2); the 4-byte spectrogram rows stay plain (see the store policy above).
#ifndef K1_SPILL_NT
#define K1_SPILL_NT 1
#endif
typedef float salsa_f4v __attribute__((ext_vector_type(4)));
#ifndef TR_NT_LD
#define TR_NT_LD 0 // probe: the tracker's read-once 8-byte loads of channel 0 as non-temporal loads
#endif
#ifndef K3_GATHER_NT
#define K3_GATHER_NT 0 // probe: the covariance kernel's 16-byte gathers as non-temporal loads (they ARE re-read: the +-3-frame halo)
#endif
typedef float salsa_f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ld_off_nt(const float4 *base, unsigned byte_off)
{
    const salsa_f4v x = __builtin_nontemporal_load((const salsa_f4v *)((const char *)base + byte_off));
    return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void st_off_nt(float4 *base, unsigned byte_off, const float4 v)
{
    salsa_f4v x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, (salsa_f4v *)((char *)base + byte_off));
}

// frames per wave.  Full SALSA: 4 (8 reuses more overlap per wave but leaves a 29 %-full last round of workgroups: measured
// 2 % slower).  SALSA-Lite, whose items are frame-major and heavier (phase rows instead of the spill): 8 (4 measured 4 % slower)
// K1_INTERLEAVE (round-5 probe): the four waves of a workgroup take frames base + w, base + w + 4, ... instead of four consecutive
// frames each, so the 212 samples per channel two consecutive frames share are requested by sibling waves at about the same time.
#ifndef K1_INTERLEAVE
#define K1_INTERLEAVE 0
#endif
#ifndef K1_NF_FULL
#define K1_NF_FULL 4
#endif
#ifndef K1_STD
#define K1_STD 1 // the STD instantiations of stft_kernel for the dataset scripts' layout (0: always the general kernel; bit-identical)
#endif
// angle(X_c conj(X_0)) of SALSA-Lite / IPD (salsa_lite_feature_extraction.py:111) in float32, with the roundings spelled out: one
// product rounded, the other fused into the sum.  Left to the compiler, `a * b + c * d` was contracted one way in the general
// instantiation and the other way in the Lite STD one (1 % of the phases differed in the last bit); every instantiation calls this.
__device__ __forceinline__ float lite_phase(const float2 xc, const float2 x0)
{
#pragma clang fp contract(off)
    float wr = fmaf(xc.x, x0.x, xc.y * x0.y);
    float wi = fmaf(xc.y, x0.x, -(xc.x * x0.y));
    const float m = fmaxf(fabsf(wr), fabsf(wi));
    if (m < 1e-30f && m > 0.f) { // products of tiny spectra: redo the product scaled up (exact)
        const float sx = 0x1p60f;
        wr = fmaf(xc.x * sx, x0.x * sx, (xc.y * sx) * (x0.y * sx));
        wi = fmaf(xc.y * sx, x0.x * sx, -((xc.x * sx) * (x0.y * sx)));
    }
    return atan2f(wi, wr);
}

// SALSA-Lite STD instantiation: channel 0's spectrum of the wave's frame, kept from the pair-0 item for the pair-1 item, lives in LDS
// (16 KB per workgroup) instead of ten registers per lane.  A function-local __shared__ array of a template that only the Lite STD
// instantiation calls, so that no other instantiation's LDS layout moves (an 8-byte dummy array cost the full-SALSA kernel 2.5 %).
constexpr int K1_LITE_X0_SLOTS = 8; // per wave: one slot per bin register (frame-major order) or per frame of the wave (pair-major order, phase band in register 0)
template <bool ON> struct k1_x0_store {
    static __device__ __forceinline__ float2 *get()
    {
        __shared__ float2 a[4 * K1_LITE_X0_SLOTS * 64];
        return a;
    }
};
template <> struct k1_x0_store<false> {
    static __device__ __forceinline__ float2 *get() { return nullptr; }
};
#ifndef K1_LITE_STD
#define K1_LITE_STD 1 // the STD instantiation of the SALSA-Lite / IPD kernel (planar 4-channel audio, n_fft 512, no scaler); 0: the general kernel (bit-identical)
#endif
#ifndef K1_LITE_PAIR_MAJOR
#define K1_LITE_PAIR_MAJOR 1 // Lite STD: pair-major item order when the phase band fits bin register 0 (0: always frame-major; bit-identical)
#endif
#ifndef K1_LITE_STD_WAVES
#define K1_LITE_STD_WAVES 3 // workgroups per CU the Lite STD instantiation is compiled for
#endif
#ifndef K1_LITE_WAVES
#define K1_LITE_WAVES 1 // workgroups per CU the SALSA-Lite / IPD instantiations are compiled for (1: no register cap -> 184 VGPRs, 2 waves per SIMD)
#endif
#ifndef K1_LITE_1024_WAVES
#define K1_LITE_1024_WAVES 1 // waves per SIMD the n_fft 1024 SALSA-Lite / IPD instantiation is compiled for (sixteen float64 points per lane: 256 VGPRs + 39 AGPRs, no scratch; capped at 2 waves = 256 registers the compiler spills 52 registers to scratch)
#endif
#ifndef K1_NF_LITE
#define K1_NF_LITE 8 // frames per wave of the SALSA-Lite / IPD instantiations
#endif
template <bool LITE> struct k1_cfg {
    static constexpr int NF = LITE ? K1_NF_LITE : K1_NF_FULL;
};

// SC (round 4): the instantiation launched when a scaler is attached keeps the [4][F] mean / std tables in LDS.  It is a separate
// instantiation because the 8 KB of LDS and the 168-register cap cost the plain path 4 % (0.458 -> 0.477 ms) when they were
// unconditional; SC = false is the round-3 kernel, bit for bit (and still honours a scaler, through global loads).
// STD (round 6, the ISA audit of profiles/r6_k1_isa.txt): the dataset scripts' spectrogram layout known at COMPILE time -- n_fft 512,
// planar audio, both channel pairs in one launch, high-frequency compression on (rows 0..191 = bins 1..192, rows 192..199 = eight
// bins each), and no scaler unless SC holds it in LDS.  Of the ~900 instructions an item issued, ~330 were not the FFT: sixteen
// load addresses rebuilt per item (the stride was a run-time value: planar | interleaved), a run-time 7-iteration tail loop in the
// compressed rows, the Nyquist bin unpacked and tested although W never reads it (:163-171), a scaler branch + division sequence
// compiled into all eleven store sites, and exec-mask juggling around band tests whose answers are fixed per register.  Same
// arithmetic in the same order: outputs are bit-identical (tests: goldens, fused-vs-three-kernel identity).  The DOA band stays a
// run-time range (FOA 1..192, MIC 1..85, any fmin / fmax).
template <int N, typename T, bool LITE, int NF, int NPAIRS = 2, bool SC = false, bool STD = false>
__global__ __launch_bounds__(256, LITE ? (STD ? K1_LITE_STD_WAVES : N == 1024 ? K1_LITE_1024_WAVES : K1_LITE_WAVES) : SC ? 3 : 1) void stft_kernel(const KParams kp, const float *__restrict__ audio,
                                                   const double *__restrict__ window,
                                                   const cplx<double> *__restrict__ tw, float *__restrict__ out,
                                                   float4 *__restrict__ Xs)
{
    constexpr int R = fft_cfg<N>::R;
    constexpr int NP = fft_cfg<N>::NP;
    constexpr int NB = N / 2 + 1;
    constexpr int NS = fft_cfg<N>::NS, NSUB = fft_cfg<N>::NSUB; // N = 1024: two NS-point transforms per item (even / odd samples)
    constexpr int RL = R * NSUB;                                 // points per lane of the N-point transform
    static_assert(NSUB == 1 || (LITE && !SC && !STD && NPAIRS == 2), "n_fft 1024 is a SALSA-Lite / IPD size only");
    __shared__ cplx<T> buf[4][NS];
    __shared__ __attribute__((aligned(16))) float pw[4][2][64]; // powers of the compressed band (<= 63 bins) of the wave's two channels (STD reads them 16 bytes at a time)

    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.y, bx = blockIdx.x;
    const int Ns = kp.N, Tn = kp.T;
    constexpr int K1_NF = NF;
    constexpr int K1_TSTEP = K1_INTERLEAVE ? 4 : 1;
    const int t_begin = K1_INTERLEAVE ? bx * 4 * K1_NF + w : (bx * 4 + w) * K1_NF;
    cplx<T> *z = buf[w];

    // Register diet (occupancy): only the first twiddle of each pass stays in registers, its powers are rebuilt by a
    // multiplication chain of depth <= 3 (relative error ~4e-16, invisible after the float32 rounding of the spectra);
    // the window (pre-scaled by the unpack's exact 1/2) is shared by the block's waves through LDS.
    __shared__ T wins[N];
    for (int i = threadIdx.x; i < N; i += 256) wins[i] = (T)(0.5 * window[i]);
    // the fused scaler's [4][F] mean / std tables, read from LDS in the store path (round 4: as global loads next to every store
    // they were a `global_load; global_load; s_waitcnt vmcnt(0)` per value -- eight exposed L2 round trips per item)
    extern __shared__ float sct_dyn[]; // SC only: [2][4 * N / 2] floats of DYNAMIC LDS (the launch passes the size), so that the plain
    float *sct0 = sct_dyn, *sct1 = sct_dyn + 4 * (N / 2); // instantiation's static LDS layout is untouched: even an 8-byte dummy
    if (SC && kp.sc_mean) {                               // array here moved the other arrays and cost the STFT 2.5 %
        for (int i = threadIdx.x; i < 4 * kp.F; i += 256) {
            sct0[i] = kp.sc_mean[i];
            sct1[i] = kp.sc_std[i];
        }
    }
    __syncthreads(); // the only workgroup barrier, before any wave-uniform exit
    cplx<T> w1[NP];
    {
        int p = R;
#pragma unroll
        for (int q = 0; q < NP; q++, p *= R) {
            const cplx<double> wd = tw[NSUB * salsa::stockham_tw(lane, 1, p, NS, R)]; // (the table holds W_N^m)
            w1[q] = {(T)wd.re, (T)wd.im};
        }
    }
    cplx<T> wj = {(T)1, (T)0}; // N = 1024: W_N^lane, the lane's part of the twiddles that join the two half transforms
    if constexpr (NSUB == 2) wj = {(T)tw[lane].re, (T)tw[lane].im};
    if (t_begin >= Tn) return; // wave-uniform; nothing below uses a workgroup barrier
    // channel pairs per clip: 2 (the dataset scripts), 3 / 4 on the contrib surface; NPAIRS == 0: any count, read from kp.nch
    // (9 - 16 microphones: one instantiation, the index arithmetic below is all that depends on it)
    const int npairs = NPAIRS > 0 ? NPAIRS : kp.nch / 2;
    const int nch = 2 * npairs;
    const float *clip = audio + (long)b * nch * Ns;
    // samples of one item: 2 channels x R strided points per lane.  Straight-line code on the (wave-uniform) interior
    // path -- no per-load branching; frames that overlap a clip end take the reflect path (np.pad(mode='reflect'); one
    // fold suffices because Ns > N/2, checked on the host).
    static_assert(!STD || (N == 512 && NPAIRS == 2 && !(LITE && SC)), "STD is the dataset scripts' configuration: n_fft 512, planar 4-channel audio");
    const bool planar = STD ? true : kp.layout == SALSA_LAYOUT_PLANAR;
    const int sstride = planar ? 1 : nch;
    // Item order.  Full SALSA: PAIR-major (all the wave's frames of channels 0/1, then of channels 2/3), so consecutive
    // items re-read the 41 % of samples that overlapping frames share while they are still in L2 (frame-major order
    // puts another 4 KiB item and a whole CU's worth of traffic in between: measured 1.7x audio over-fetch).  SALSA-Lite
    // needs channel 0 of the same frame when it processes pair 1, so it stays frame-major.
#if defined(K1_FRAME_MAJOR)
    constexpr bool PAIR_MAJOR = false;
#else
    constexpr bool PAIR_MAJOR = !LITE;
#endif
    const int nleft_ = (Tn - t_begin + K1_TSTEP - 1) / K1_TSTEP; // frames t_begin, t_begin + K1_TSTEP, ... below Tn
    const int nfr_ = STD ? __builtin_amdgcn_readfirstlane(nleft_ < K1_NF ? nleft_ : K1_NF) : (nleft_ < K1_NF ? nleft_ : K1_NF);
    const int psel = (LITE || STD) ? -1 : kp.pair_sel; // one channel pair per launch (the pipelined schedule): item = frame
    // Lite STD: when every bin whose phase survives :120 sits in bin register 0 (lower + upper <= 64: the dataset script's fmax_doa 2000
    // gives bins 1..42), channel 0 of a frame is 512 B per wave and the wave's whole run of frames fits in LDS: PAIR-major order like
    // full SALSA (the frame-major order re-read the samples neighbouring frames share from HBM: 1.6x the audio, profiles/r6_ab_notes.txt)
    const bool lite_pm = (LITE && STD && K1_LITE_PAIR_MAJOR) ? (64 - kp.lower >= kp.upper && K1_NF <= K1_LITE_X0_SLOTS) : false;
    auto item_frame = [&](int item) {
        if (NPAIRS != 2) return PAIR_MAJOR ? item % nfr_ : item / npairs;
        if (LITE && STD) return lite_pm ? (item >= nfr_ ? item - nfr_ : item) : item >> 1;
        return psel >= 0 ? item : PAIR_MAJOR ? (item >= nfr_ ? item - nfr_ : item) : item >> 1;
    };
    auto item_pair = [&](int item) {
        if (LITE && STD && NPAIRS == 2) return lite_pm ? (item >= nfr_ ? 1 : 0) : item & 1;
        if (NPAIRS != 2) return PAIR_MAJOR ? item / nfr_ : item % npairs;
        return psel >= 0 ? psel : PAIR_MAJOR ? (item >= nfr_ ? 1 : 0) : item & 1;
    };
    auto load_item = [&](int item, float *y0, float *y1) {
        const int t = t_begin + K1_TSTEP * item_frame(item);
        const int c0 = 2 * item_pair(item);
        const int base = t * kp.hop - N / 2;
        const unsigned ch0 = 4u * (unsigned)(planar ? c0 * Ns : c0), ch1 = ch0 + 4u * (unsigned)(planar ? Ns : 1); // byte offsets
        const unsigned step = 4u * (unsigned)sstride;
        if (base >= 0 && base + N <= Ns) {
            const unsigned q = (unsigned)(base + NSUB * lane) * step;
#pragma unroll
            for (int u = 0; u < NSUB; u++)
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (STD) { // planar, 4-byte stride: the eight strided points of a channel are one address + immediates r * 256 (tried for every
                           // planar plan behind a wave-uniform branch: the general instantiations went from 168 to 174 VGPRs = 2 waves per SIMD)
                    y0[r] = ld_off_c(clip, ch0 + q, r * (N / R) * 4);
                    y1[r] = ld_off_c(clip, ch1 + q, r * (N / R) * 4);
                } else {
                    y0[u * R + r] = ld_off(clip, ch0 + q + (unsigned)(NSUB * r * (NS / R) + u) * step); // (sub-transform u: samples u, u + NSUB, ...)
                    y1[u * R + r] = ld_off(clip, ch1 + q + (unsigned)(NSUB * r * (NS / R) + u) * step);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < NSUB; u++)
#pragma unroll
            for (int r = 0; r < R; r++) {
                int s = base + NSUB * salsa::stockham_in(lane, r, NS, R) + u;
                s = s < 0 ? -s : s;
                s = s >= Ns ? 2 * (Ns - 1) - s : s;
                y0[u * R + r] = ld_off(clip, ch0 + (unsigned)s * step);
                y1[u * R + r] = ld_off(clip, ch1 + (unsigned)s * step);
            }
        }
    };

    const int nitems = psel >= 0 ? nfr_ : nfr_ * npairs;
    float y0[RL], y1[RL];
    float *o = out + (long)b * kp.OC * Tn * kp.F; // [OC][T][F] of this clip (int offsets below)
    float4 *xs = Xs + (long)b * Tn * npairs * kp.nd;
    const int mlane = (64 - lane) & 63;           // lane holding the mirror bins N-k of this lane's bins
    // log-spectrogram value of channel c, feature f; with a scaler attached also (x - mean) / std (database.py:197-202)
    auto spec = [&](const float p, const int c, const int f) -> float {
        const float v = db10(p);
        if (STD && !SC) return v;                 // (the launch guarantees: no scaler attached)
        if (SC) {
            const int i = c * kp.F + f;
            return kp.sc_mean ? (v - sct0[i]) / sct1[i] : v;
        }
        const unsigned off = 4u * (unsigned)(c * kp.F + f);
        return kp.sc_mean ? (v - ld_off(kp.sc_mean, off)) / ld_off(kp.sc_std, off) : v;
    };
    const unsigned plane = 4u * (unsigned)(Tn * kp.F); // bytes of one output channel of a clip
    float2 x0keep[(LITE && STD) ? 1 : RL / 2 + 1]; // SALSA-Lite: channel-0 spectrum of this lane's bins, kept from pair 0 for pair 1 (Lite STD: in LDS)
    float2 *const x0s = k1_x0_store<LITE && STD>::get() + (LITE && STD ? w * K1_LITE_X0_SLOTS * 64 + lane : 0);

    for (int item = 0; item < nitems; item++) {
        const int t = t_begin + K1_TSTEP * item_frame(item);
        const int pr = item_pair(item);
        load_item(item, y0, y1);
        cplx<T> v[RL];
#pragma unroll
        for (int u = 0; u < NSUB; u++)
#pragma unroll
        for (int r = 0; r < R; r++) {
            const T wn = wins[NSUB * salsa::stockham_in(lane, r, NS, R) + u];
            v[u * R + r] = {wn * (T)y0[u * R + r], wn * (T)y1[u * R + r]};
        }
        // ---- Stockham passes, in place in the wave-private buffer (N = 1024: the even samples' transform, then the odd samples')
#pragma unroll
        for (int u = 0; u < NSUB; u++) {
            cplx<T> *const vs = v + u * R;
            salsa::dftR<R>(vs); // pass p = 1 (no twiddles)
#pragma unroll
            for (int r = 0; r < R; r++) z[swz(salsa::stockham_out(lane, r, 1, R))] = vs[r];
            {
                int p = R;
#pragma unroll
                for (int q = 0; q < NP; q++, p *= R) {
                    wave_lds_fence();
#pragma unroll
                    for (int r = 0; r < R; r++) vs[r] = z[swz(salsa::stockham_in(lane, r, NS, R))];
                    wave_lds_fence();
                    {
                        const cplx<T> a1 = w1[q], a2 = salsa::cmul(a1, a1), a3 = salsa::cmul(a2, a1);
                        vs[1] = salsa::cmul(vs[1], a1);
                        vs[2] = salsa::cmul(vs[2], a2);
                        vs[3] = salsa::cmul(vs[3], a3);
                        if (R == 8) {
                            const cplx<T> a4 = salsa::cmul(a2, a2);
                            vs[4 % R] = salsa::cmul(vs[4 % R], a4);
                            vs[5 % R] = salsa::cmul(vs[5 % R], salsa::cmul(a4, a1));
                            vs[6 % R] = salsa::cmul(vs[6 % R], salsa::cmul(a3, a3));
                            vs[7 % R] = salsa::cmul(vs[7 % R], salsa::cmul(a4, a3));
                        }
                    }
                    salsa::dftR<R>(vs);
                    if (q + 1 < NP) {
#pragma unroll
                        for (int r = 0; r < R; r++) z[swz(salsa::stockham_out(lane, r, p, R))] = vs[r];
                    }
                }
            }
        }
        if constexpr (NSUB == 2) {
            // join: lane holds E[lane + 64 r] in v[r] and O[lane + 64 r] in v[R + r]; Z[k] = E[k] + W_N^k O[k], Z[k + N/2] = E[k] - W_N^k O[k]
            // with W_N^(lane + 64 r) = W_N^lane * W_16^r
            static_assert(R == 8, "the join's constants are W_16^r");
            constexpr double c16[8] = {1.0, 0.92387953251128675613, 0.70710678118654752440, 0.38268343236508977173,
                                       0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613};
            constexpr double s16[8] = {0.0, -0.38268343236508977173, -0.70710678118654752440, -0.92387953251128675613,
                                       -1.0, -0.92387953251128675613, -0.70710678118654752440, -0.38268343236508977173};
#pragma unroll
            for (int r = 0; r < R; r++) {
                const cplx<T> wk = r == 0 ? wj : salsa::cmul(wj, cplx<T>{(T)c16[r], (T)s16[r]});
                const cplx<T> e = v[r], ow = salsa::cmul(v[R + r], wk);
                v[r] = salsa::cadd(e, ow);
                v[R + r] = salsa::csub(e, ow);
            }
        }
        // lane now holds Z[lane + 64 r] in v[r] (the last pass writes y[i + r*64])

        // ---- unpack this pair's two spectra: bins k = lane + 64 r, r < R/2 (+ lane 0: the Nyquist bin)
        const int c0 = 2 * pr;
        auto emit_bin = [&](const int k, const cplx<T> a, const cplx<T> bm, float2 &x0k) {
            cplx<T> Xa, Xb;
            salsa::unpack_pair_prescaled(a, bm, Xa, Xb);
            const float2 xa = make_float2((float)Xa.re, (float)Xa.im); // the reference stores its STFT as complex64
            const float2 xb = make_float2((float)Xb.re, (float)Xb.im);
            const float pa = power32(xa), pb = power32(xb);
            if (!LITE) {
                if (kp.feature == SALSA_FEATURE_SALSA && k >= kp.lower && k < kp.upper)
                {
                    const unsigned so = 16u * (unsigned)((t * npairs + pr) * kp.nd + (k - kp.lower));
                    if (K1_SPILL_NT) st_off_nt(xs, so, make_float4(xa.x, xa.y, xb.x, xb.y));
                    else st_off(xs, so, make_float4(xa.x, xa.y, xb.x, xb.y));
                }
                if (k >= kp.spec_lo && k < kp.spec_hi) {
                    const unsigned off = 4u * (unsigned)((c0 * Tn + t) * kp.F + (k - kp.spec_lo));
                    st_off(o, off, spec(pa, c0, k - kp.spec_lo));
                    st_off(o, off + plane, spec(pb, c0 + 1, k - kp.spec_lo));
                } else if (kp.compress && k > kp.ident && k < N / 2) {
                    pw[w][0][k - kp.ident - 1] = pa;
                    pw[w][1][k - kp.ident - 1] = pb;
                }
            } else { // SALSA-Lite / SALSA-IPD (salsa_lite_feature_extraction.py:103-120)
                if (pr == 0) x0k = xa;
                if (k >= kp.lower && k < kp.cutoff) {
                    const int f = k - kp.lower;
                    const unsigned off = 4u * (unsigned)((c0 * Tn + t) * kp.F + f);
                    st_off(o, off, spec(pa, c0, f));
                    st_off(o, off + plane, spec(pb, c0 + 1, f));
                    const float2 x0 = x0k;
                    // angle(X_c conj(X_0)) / (delta*k) (lite :111-115) or / pi (ipd :113).  float32 throughout: the
                    // product's rounding moves the angle by <= 1e-7 rad and 1/(delta*k) is the float64 quotient rounded
                    // once, so the float32 result is within ~2 ulp of the reference's float64-then-cast value.
                    // (contrib's float32 frequency vector differs from delta*k by <= 6e-8 relative: same float32 result)
                    const float inv_scale = kp.feature == SALSA_FEATURE_IPD ? 0.318309886183790672f
                                                                           : (float)(1.0 / (kp.delta * (double)(k == 0 ? 1 : k)));
                    // pair 0 contributes channel 1 (phase vs channel 0); pair p >= 1 contributes channels 2p and 2p+1: the phase of
                    // channel c goes to output plane NCH + c - 1, i.e. NCH - 1 and NCH planes above this pair's spectrogram
                    auto phase = [&](const float2 xc) -> float {
                        if (!(f < kp.upper)) return 0.f; // ":120 phase_vector[:, :, upper_bin:] = 0" indexes the CROPPED axis
                        return lite_phase(xc, x0) * inv_scale;
                    };
                    if (pr >= 1) st_off(o, off + (unsigned)(nch - 1) * plane, phase(xa));
                    st_off(o, off + (unsigned)nch * plane, phase(xb));
                }
            }
        };
        // STD: register r holds bins 64 r .. 64 r + 63, so with spec_lo = 1, spec_hi = 193, ident = 192 the spectrogram-row / compressed-
        // band membership of a bin is fixed per register: r = 0 -- rows for every lane but lane 0 (bin 0: W has no row for it);
        // r = 1, 2 -- rows, all lanes; r = 3 -- lane 0 is bin 192 (row 191), lanes 1..63 are bins 193..255 of the compressed rows.
        auto emit_std = [&](auto rc, const cplx<T> a, const cplx<T> bm) {
            constexpr int r = decltype(rc)::value;
            const int k = lane + 64 * r;
            cplx<T> Xa, Xb;
            salsa::unpack_pair_prescaled(a, bm, Xa, Xb);
            const float2 xa = make_float2((float)Xa.re, (float)Xa.im);
            const float2 xb = make_float2((float)Xb.re, (float)Xb.im);
            const float pa = power32(xa), pb = power32(xb);
            if (k >= kp.lower && k < kp.upper) {
                const unsigned so = 16u * (unsigned)((t * 2 + pr) * kp.nd + (k - kp.lower));
                if (K1_SPILL_NT) st_off_nt(xs, so, make_float4(xa.x, xa.y, xb.x, xb.y));
                else st_off(xs, so, make_float4(xa.x, xa.y, xb.x, xb.y));
            }
            if (r < 3 ? (r > 0 || lane > 0) : lane == 0) {
                const unsigned off = 4u * (unsigned)((c0 * Tn + t) * 200 + (k - 1));
                st_off(o, off, spec(pa, c0, k - 1));
                st_off(o, off + plane, spec(pb, c0 + 1, k - 1));
            } else if (r == 3) {
                pw[w][0][lane - 1] = pa;
                pw[w][1][lane - 1] = pb;
            }
        };
        // Lite STD: same arithmetic as emit_bin's SALSA-Lite branch.  What is fixed per register here: register r holds bins 64 r .. 64 r + 63,
        // so whether it has any bin below the cutoff, and any bin whose phase is not zeroed by :120, are wave-uniform tests (scalar
        // branches around whole blocks instead of exec-masked code); channel 0's spectrum goes through LDS; no Nyquist item.
        auto emit_lite_std = [&](auto rc, const cplx<T> a, const cplx<T> bm) {
            constexpr int r = decltype(rc)::value;
            if (64 * r >= kp.cutoff) return;                       // wave-uniform: no bin of this register is written
            const bool any_phase = 64 * r - kp.lower < kp.upper;   // wave-uniform: some bin of this register keeps its phase (:120)
            const int k = lane + 64 * r;
            cplx<T> Xa, Xb;
            salsa::unpack_pair_prescaled(a, bm, Xa, Xb);
            const float2 xa = make_float2((float)Xa.re, (float)Xa.im); // the reference stores its STFT as complex64
            const float2 xb = make_float2((float)Xb.re, (float)Xb.im);
            const float pa = power32(xa), pb = power32(xb);
            float2 x0 = xa;
            if (any_phase) { // (pair-major order: only register 0 comes here, the slot is the frame's place in the wave's run)
                const int slot = lite_pm ? item_frame(item) : r;
                if (pr == 0) x0s[slot * 64] = xa;
                else x0 = x0s[slot * 64];
            }
            if (k >= kp.lower && k < kp.cutoff) {
                const int f = k - kp.lower;
                const unsigned off = 4u * (unsigned)((c0 * Tn + t) * kp.F + f);
                st_off(o, off, db10(pa));
                st_off(o, off + plane, db10(pb));
                float pha = 0.f, phb = 0.f;
                if (any_phase) {
                    const float inv_scale = kp.feature == SALSA_FEATURE_IPD ? 0.318309886183790672f
                                                                           : (float)(1.0 / (kp.delta * (double)(k == 0 ? 1 : k)));
                    auto phase = [&](const float2 xc) -> float {
                        if (!(f < kp.upper)) return 0.f; // ":120 phase_vector[:, :, upper_bin:] = 0" indexes the CROPPED axis
                        return lite_phase(xc, x0) * inv_scale;
                    };
                    if (pr >= 1) pha = phase(xa);
                    phb = phase(xb);
                }
                if (pr >= 1) st_off(o, off + 3u * plane, pha);
                st_off(o, off + 4u * plane, phb);
            }
        };
#pragma unroll
        for (int r = 0; r < RL / 2; r++) {
            // mirror of k = lane + 64 r is N-k = (64-lane) + 64 (RL-1-r): register RL-1-r of lane 64-lane;
            // lane 0: N - 64 r = 64 (RL-r), its own register (RL-r) mod RL
            if constexpr (NSUB == 2) {
                if (64 * r >= kp.cutoff) continue; // wave-uniform: no bin of this register is written (nor its X0 read: emit_bin)
            }
            cplx<T> bm = {__shfl(v[RL - 1 - r].re, mlane), __shfl(v[RL - 1 - r].im, mlane)};
            if (lane == 0) bm = v[(RL - r) & (RL - 1)];
            if constexpr (STD && LITE) {
                if (r == 0) emit_lite_std(std::integral_constant<int, 0>{}, v[r], bm);
                else if (r == 1) emit_lite_std(std::integral_constant<int, 1>{}, v[r], bm);
                else if (r == 2) emit_lite_std(std::integral_constant<int, 2>{}, v[r], bm);
                else emit_lite_std(std::integral_constant<int, 3>{}, v[r], bm);
            } else if constexpr (STD) {
                if (r == 0) emit_std(std::integral_constant<int, 0>{}, v[r], bm);
                else if (r == 1) emit_std(std::integral_constant<int, 1>{}, v[r], bm);
                else if (r == 2) emit_std(std::integral_constant<int, 2>{}, v[r], bm);
                else emit_std(std::integral_constant<int, 3>{}, v[r], bm);
            } else {
                emit_bin(lane + 64 * r, v[r], bm, x0keep[(LITE && STD) ? 0 : r]);
            }
            __builtin_amdgcn_sched_barrier(0); // one bin at a time: keeps the live set (and the VGPR count) small
        }
        if (!STD && lane == 0) emit_bin(N / 2, v[RL / 2], v[RL / 2], x0keep[(LITE && STD) ? 0 : RL / 2]); // (STD: bin 256 is in no DOA band, row or compressed row)
        // ---- compressed high-frequency rows of W: sum of 8 (last row 7) bins times 1/8
        if constexpr (STD && !LITE) {
            // eight groups x two channels = lanes 0..15: two 16-byte LDS reads and a fixed chain of eight additions in the order of
            // the loop below (the seventh row's missing eighth term is skipped, not added as zero: pw[..][63] is never written)
            wave_lds_fence();
            const int h = lane & 1, gi = lane >> 1;
            if (gi < 8) {
                const float4 p0 = *(const float4 *)&pw[w][h][8 * gi], p1 = *(const float4 *)&pw[w][h][8 * gi + 4];
                float acc = 0.f;
                acc += 0.125f * p0.x; acc += 0.125f * p0.y; acc += 0.125f * p0.z; acc += 0.125f * p0.w;
                acc += 0.125f * p1.x; acc += 0.125f * p1.y; acc += 0.125f * p1.z;
                const float acc8 = acc + 0.125f * p1.w;
                acc = gi < 7 ? acc8 : acc;
                st_off(o, 4u * (unsigned)(((c0 + h) * Tn + t) * 200 + 192 + gi), spec(acc, c0 + h, 192 + gi));
            }
        } else if (!LITE && kp.compress) {
            wave_lds_fence();
            const int ng = kp.F - kp.ident;
            const int h = lane & 1, gi = lane >> 1;
            if (gi < ng) {
                const int cnt = gi < ng - 1 ? 8 : 7;
                float acc = 0.f;
                for (int q = 0; q < cnt; q++) acc += 0.125f * pw[w][h][8 * gi + q];
                st_off(o, 4u * (unsigned)(((c0 + h) * Tn + t) * kp.F + kp.ident + gi), spec(acc, c0 + h, kp.ident + gi));
            }
        }
        wave_lds_fence(); // this item's LDS reads are done before the next item's first pass overwrites z / pw
    }
}

// ------------------------------------------------------------------------------------------------------------ K2
// Noise-floor tracker.  The recurrence over time is strictly sequential per (clip, bin), but everything that feeds it
// (|X0|^2, the 3-frame mean, the float64 divide and square root) is not: producer waves stay one chunk of TR_CH frames
// ahead of the consumer wave, computing mag[t][bin] into an LDS ring.  Spill layout: Xs[b][t][pair][bin] as float4
// (c0.re, c0.im, c1.re, c1.im); channel 0 is the .xy of pair 0.  Output: valid32[b][32-bin group][t] = indicator_sig mask
// of frame t (bit j = bin 32*group + j).
#ifndef TR_WAVES_N
#define TR_WAVES_N 8
#endif
constexpr int TR_WAVES = TR_WAVES_N; // wave 0 = consumer; with more than 4 waves, wave 4 idles (see tracker_kernel); the rest produce

template <int COUNT>
__device__ __forceinline__ void tracker_load(const KParams &kp, const float4 *__restrict__ x0, int stride, int c0,
                                             int first, bool active, float2 *x)
{
    // |X0| samples of frames c0+first-2 .. c0+first+COUNT-1 (wrap on the time axis; beyond the clip: unused)
    const int Tn = kp.T;
#pragma unroll
    for (int i = 0; i < COUNT + 2; i++) {
        int t = c0 + first + i - 2;
        if (t >= Tn) t = Tn - 1;
        while (t < 0) t += Tn;
        if (TR_NT_LD) {
            const salsa_f2v v = active ? __builtin_nontemporal_load((const salsa_f2v *)&x0[t * stride]) : salsa_f2v{0.f, 0.f};
            x[i] = make_float2(v.x, v.y);
        } else
            x[i] = active ? *(const float2 *)&x0[t * stride] : make_float2(0.f, 0.f); // channel 0 = .xy of pair 0
    }
}

// x / 3 correctly rounded (= the reference's float64 division, :53-55) in three instructions instead of the ~14 of the compiler's
// IEEE division sequence (two v_div_scale, a quarter-rate v_rcp_f64, five FMAs, v_div_fmas, v_div_fixup): with y = RN(1/3) and
// q = RN(x y) faithful, the residual r = x - 3 q is exact in one FMA and RN(q + r y) is the correctly rounded quotient (Markstein's
// theorem; checked against exact rational arithmetic on 7e5 values incl. subnormals, tools/probes/div3_check.py).  The tracker's
// producer waves do one division and one square root per (frame, bin): 29 M of each per 32-clip batch.
#ifndef TR_DIV3_EXACT
#define TR_DIV3_EXACT 1
#endif
__device__ __forceinline__ double div3_exact(const double x)
{
#if TR_DIV3_EXACT
    const double y = 1.0 / 3.0; // RN(1/3), a compile-time constant
    const double q = x * y;
    const double r = __builtin_fma(-3.0, q, x);
    return __builtin_fma(r, y, q);
#else
    return x / 3;
#endif
}

template <int COUNT, int BINS>
__device__ __forceinline__ void tracker_mag(const float2 *x, int first, double *dst /*[TR_CH][BINS]*/, int col, bool raw)
{
    double p[COUNT + 2];
#pragma unroll
    for (int i = 0; i < COUNT + 2; i++) {
        const double re = x[i].x, im = x[i].y;
        p[i] = re * re + im * im;
    }
#pragma unroll
    for (int i = 0; i < COUNT; i++) {
        if (first + i < TR_CH) // :53-55 in the reference's order ; contrib :326-328 tracks the raw |X0| instead
            dst[(first + i) * BINS + col] = raw ? sqrt(p[i + 2]) : sqrt(div3_exact(((0.0 + p[i + 2]) + p[i + 1]) + p[i]));
    }
}

// One workgroup = 32 adjacent bins of one clip, TR_WAVES waves: wave 0 is the CONSUMER (the recurrence), the others are
// producers.  What bounds this kernel is the consumer: 4801 strictly sequential steps per clip of ~16 instructions each, issued
// by ONE wave -- so everything is arranged for that wave's issue rate and dependent-chain latency:
//  * a wave issues at most one instruction per 4-cycle slot of its SIMD, so the step costs ~4.5 cycles x its instruction count
//    (17 here, 23 in round 1) -- PROVIDED the consumer has its SIMD to itself.  A workgroup's waves go to the four SIMDs
//    cyclically, so wave 4 would share the consumer's: it does nothing but the barriers (a wave parked at s_barrier takes no
//    issue slots) and the six producers are waves 1-3 and 5-7.  They need ~440 cycles per (2 frames x 32 bins) item -- the
//    float64 divide and square root are quarter-rate -- i.e. ~2700 cycles per chunk against the consumer's ~4900;
//  * the step's dependent chain is  multiply -> select -> max  (salsa::tracker_step forms both candidate products first);
//  * indicator_sig never becomes a per-lane value: the compare writes a scalar lane mask (one bit per bin), which is exactly
//    the per-frame mask the covariance kernel wants; v_writelane drops it into lane `frame` of one VGPR and the chunk's 64
//    masks leave as ONE coalesced 256-byte store: valid32[b][32-bin group][t].  (Round 1 shifted a bit into a per-bin history
//    word -- three VALU instructions per step -- and K3 had to ballot the words back into frame masks.)
//  * all 64 lanes run the recurrence (lanes 32-63 mirror 0-31), so the consumer has no divergent region around the writelanes;
//  * producers keep TWO register sets of spectra and alternate them (the chunk loop is unrolled by two): the loads issued in
//    one iteration are first used in the next, a whole chunk later.  (Round 1 copied "next" into "current" at the end of every
//    iteration, which made each iteration wait for the loads it had just issued.)
#ifndef TR_IDLE4
#define TR_IDLE4 1
#endif
#ifndef TR_MASK_HISTORY
#define TR_MASK_HISTORY 1 // the countdown as three scalar `above` masks (round 3); 0: the per-lane countdown of round 2
#endif
#ifndef TR_CHUNK_CLAMP_SKIP
#define TR_CHUNK_CLAMP_SKIP 0 // round 5: chunks whose floors cannot reach the 1e-6 clamp run the step without it (see the consumer).
                              // Masks bit-identical (20 GPU parity tests), tracker 0.175 - 0.183 (off) vs 0.180 - 0.188 ms (on): no gain, off
#endif
#ifndef TR_LAZY_CLAMP
#define TR_LAZY_CLAMP 0 // measured: 0.35 ms with the lazy clamp against 0.22 ms without -- the chain is not what bounds the step
#endif
// v_writelane_b32 through the LLVM intrinsic (this clang has no __builtin for it).  Not inline asm: a VALU compare that writes
// VCC needs two wait states before v_writelane may read it, and only the compiler's hazard recogniser inserts them -- the
// hand-written form read stale masks in 0.7 % of the frames.
extern "C" __device__ int salsa_writelane_i32(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");
// TR_WIDE (round-3 review: "give the consumer 64 distinct bins per wave and report what that does"): a workgroup serves 64 bins,
// lanes 32-63 run bins 32-63 instead of mirroring lanes 0-31, a frame's ballot is two mask words.  Measured (profiles/r4_ab_notes.txt):
// see there; the mask layout valid32[b][32-bin group][t] is unchanged.
#ifndef TR_WIDE
#define TR_WIDE 0
#endif
constexpr int TR_WG_BINS = TR_WIDE ? 64 : TR_BINS;
static unsigned tracker_grid(const KParams &kp) { return (unsigned)(kp.B * ((kp.nd + TR_WG_BINS - 1) / TR_WG_BINS)); }

__global__ __launch_bounds__(64 * TR_WAVES) void tracker_kernel(const KParams kp, const float4 *__restrict__ Xs,
                                                                unsigned *__restrict__ valid32)
{
    if (kp.doubt_flag && blockIdx.x == 0 && threadIdx.x == 0) *kp.doubt_flag = 0u; // (consumed two launches later, same stream)
    constexpr int BINS = TR_WG_BINS, FS = 64 / BINS;                                      // FS frames per producer instruction
    constexpr bool IDLE4 = TR_WAVES > 4 && TR_IDLE4;                                     // wave 4 shares the consumer's SIMD: keep it idle
    constexpr int NPROD = IDLE4 ? TR_WAVES - 2 : TR_WAVES - 1;
    constexpr int PER_ALL = (TR_CH + TR_WAVES * FS - 1) / (TR_WAVES * FS);               // prologue: all waves produce chunk 0
    constexpr int PER_PROD = (TR_CH + NPROD * FS - 1) / (NPROD * FS);                    // frames per producer lane per chunk
    __shared__ double ring[2][TR_CH * BINS];
    const int ng32 = (kp.nd + BINS - 1) / BINS;
    const int b = blockIdx.x / ng32, g = blockIdx.x % ng32;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int col = lane % BINS, fsub = lane / BINS;            // producers: lane = (frame sub-slot, bin column)
    const int bin = g * BINS + col;
    const bool active = bin < kp.nd;
    const int Tn = kp.T;
    const int stride = (kp.nch / 2) * kp.nd; // float4 elements per frame (one per channel pair and bin)
    const float4 *x0 = Xs + (long)b * Tn * stride + (active ? bin : 0);
    const int nchunks = (Tn + TR_CH - 1) / TR_CH;
    const bool raw = kp.flex != 0;
    {
        float2 x[PER_ALL + 2];
        const int first = (w * FS + fsub) * PER_ALL;
        tracker_load<PER_ALL>(kp, x0, stride, 0, first, active, x);
        tracker_mag<PER_ALL, BINS>(x, first, ring[0], col, raw);
    }
    float2 xa[PER_PROD + 2], xb[PER_PROD + 2];
    const bool producer = w > 0 && !(IDLE4 && w == 4);
    const int pidx = (IDLE4 && w > 4) ? w - 2 : w - 1;           // producer number 0 .. NPROD-1
    const int pfirst = (pidx * FS + fsub) * PER_PROD;
    if (producer && nchunks > 1) tracker_load<PER_PROD>(kp, x0, stride, TR_CH, pfirst, active, xa);
    __syncthreads();
    // Consumer state: noise floor + countdown (salsa_feature_extraction.py:30, :58), evaluated with exactly the reference's
    // operations (one float64 multiply by 1.02 / 1.002 / 0.98, the 1e-6 clamp, the two strict compares).
    double fl = 0.0;
    int cd = 3;
    const double snr = kp.snr_ratio;
    const int n32 = (kp.nd + TR_BINS - 1) / TR_BINS;      // 32-bin mask groups of a clip
    unsigned *vout = valid32 + ((long)b * n32 + (TR_WIDE ? 2 * g : g)) * Tn; // [b][32-bin group][t]
    unsigned *vout_hi = (TR_WIDE && 2 * g + 1 < n32) ? vout + Tn : nullptr;     // TR_WIDE: the group of bins 32-63 of this workgroup
#if TR_MASK_HISTORY
    // Round 3: the countdown never becomes a per-lane value either.  "countdown < 1 before this step's decrement" (:68-69: the
    // slow rise) holds exactly when the three steps before this one were all `above` (the countdown starts at 3, every `above`
    // takes one off, anything else puts it back to 3), and `above` is already a scalar lane mask -- the float64 compare writes
    // one.  So the state is three 64-bit masks in SGPRs, the test is two s_and_b64 on the scalar unit, and
    // __builtin_amdgcn_inverse_ballot hands the result to v_cndmask as its mask operand: the three VALU instructions of the
    // per-lane countdown (compare, reset-select, decrement) are gone, and with them the reason to form BOTH candidate products --
    // the factor (1.02 | 1.002 | 0.98) is selected and multiplied once, the same single multiplication the reference does.
    // 14 -> 10 vector instructions per step.  Measured (tools/probes/f64_latency_probe.hip, the probe builds TR_PROBE_NO_*): the
    // consumer wave alone is 0.158 of the kernel's 0.177 ms, and its step time follows its INSTRUCTION COUNT (~7.6 cycles per
    // vector instruction of this mix: VOP3 compares writing SGPR pairs, selects reading them), not the dependent chain -- a
    // hand-pipelined order that puts the indicator of step t-1 into the stall slots of step t's chain ran no faster (0.179).
    unsigned long long h1 = 0ull, h2 = 0ull, h3 = 0ull; // `above` masks of the previous three steps (wave-uniform)
    // CLAMPED = false (round 5): the 1e-6 clamp (:85) left out.  The floor falls by at most 0.98 per step, so a chunk that STARTS
    // with every lane's floor >= 1e-6 / 0.98^64 (3.65e-6; 4e-6 is tested) cannot bring any floor below 1e-6 within its 64 steps:
    // max(x, 1e-6) == x bit for bit there, and the chunk runs 9 instead of 10 vector instructions per step with the float64 max
    // off the dependent chain.  Near-silent bins (a floor at the clamp) take the clamped step; the test is one ballot per chunk.
    auto step = [&](const double m, auto clamped) -> unsigned long long {
        const bool slow = __builtin_amdgcn_inverse_ballot_w64(h1 & h2 & h3);
        const double up = slow ? 1.0 + 0.1 * 0.02 : 1.0 + 0.02;
        const bool above = m > fl;
        const double f = above ? up : 1.0 - 0.02;
        if (decltype(clamped)::value) fl = fmax(f * fl, 1e-6); // (a product of finite numbers is canonical: one v_max_f64)
        else fl = f * fl;
        h3 = h2;
        h2 = h1;
        h1 = __ballot(above);
        return __ballot(m > snr * fl); // :87
    };
#else
    auto step = [&](const double m, auto) -> unsigned long long { return __ballot(salsa::tracker_step(fl, cd, m, snr)); }; // :65-87
#endif
    auto consume = [&](const int c) {
        const double *cur = ring[c & 1] + col;
        if (c == 0) { // noise_floor = 0.5 * mean(mag[0:5])  (:58)
            const int n0 = Tn < 5 ? Tn : 5;
            double acc = 0.0;
            for (int t = 0; t < n0; t++) acc += cur[t * BINS];
            fl = 0.5 * (acc / (double)n0);
            if (kp.flex && fl < 1e-6) fl = 1e-6; // contrib's tracker clamps its initial floor (:118-120)
        }
        unsigned word = 0, word_hi = 0; // lane i: indicator_sig mask (bit j = bin 32 g + j) of frame 64 c + i (TR_WIDE: + bins 32-63)
        const int nfr = Tn - c * TR_CH < TR_CH ? Tn - c * TR_CH : TR_CH; // wave-uniform
        if (nfr == TR_CH) { // every chunk but the last: straight-line code, no per-frame conditionals
#if TR_MASK_HISTORY
            const bool noclamp = __ballot(!(fl >= 4e-6)) == 0ull; // wave-uniform: no lane's floor can reach the clamp in this chunk
#else
            const bool noclamp = false;
#endif
#pragma unroll
            for (int i0 = 0; i0 < TR_CH; i0 += 16) {
                double m[16]; // one LDS round trip per 16 frames, not per frame
#pragma unroll
                for (int i = 0; i < 16; i++) m[i] = cur[(i0 + i) * BINS];
#if TR_LAZY_CLAMP && !TR_MASK_HISTORY
                // The 1e-6 clamp (:85) is a float64 max on the step's dependent chain (multiply -> select -> max), yet it only
                // ever acts on near-silent bins.  So a block of 16 steps runs WITHOUT it, a running minimum of the floor rides
                // along off the chain, and only if some lane's floor dipped below 1e-6 (wave-uniform test) the block is redone
                // from its saved state with the clamp.  Where no clamp acts max(x, 1e-6) == x, so the result is bit-identical.
                const double fl0 = fl;
                const int cd0 = cd;
                const unsigned word0 = word;
                double mn = fl;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const unsigned long long bal = __ballot(salsa::tracker_step<false>(fl, cd, m[i], snr)); // :65-87
                    asm("v_min_f64 %0, %0, %1" : "+v"(mn) : "v"(fl)); // (fmin() would canonicalise its operand first: one more float64 op)
                    word = (unsigned)salsa_writelane_i32((int)(unsigned)bal, i0 + i, (int)word);
                }
                if (__ballot(mn < 1e-6) != 0ull) {
                    fl = fl0;
                    cd = cd0;
                    word = word0;
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const unsigned long long bal = __ballot(salsa::tracker_step<true>(fl, cd, m[i], snr));
                        word = (unsigned)salsa_writelane_i32((int)(unsigned)bal, i0 + i, (int)word);
                    }
                }
#else
                if (TR_CHUNK_CLAMP_SKIP && noclamp) {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const unsigned long long bal = step(m[i], std::false_type{});
                        word = (unsigned)salsa_writelane_i32((int)(unsigned)bal, i0 + i, (int)word);
                        if (TR_WIDE) word_hi = (unsigned)salsa_writelane_i32((int)(unsigned)(bal >> 32), i0 + i, (int)word_hi);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        const unsigned long long bal = step(m[i], std::true_type{});
                        word = (unsigned)salsa_writelane_i32((int)(unsigned)bal, i0 + i, (int)word);
                        if (TR_WIDE) word_hi = (unsigned)salsa_writelane_i32((int)(unsigned)(bal >> 32), i0 + i, (int)word_hi);
                    }
                }
#endif
            }
        } else {
            for (int i = 0; i < nfr; i++) {
                const unsigned long long bal = step(cur[i * BINS], std::true_type{});
                word = lane == i ? (unsigned)bal : word; // (ragged last chunk only)
                if (TR_WIDE) word_hi = lane == i ? (unsigned)(bal >> 32) : word_hi;
            }
        }
        if (lane < nfr) vout[c * TR_CH + lane] = word;
        if (TR_WIDE && vout_hi && lane < nfr) vout_hi[c * TR_CH + lane] = word_hi;
    };
    // producers, iteration c: issue the loads of chunk c+2 into `nxt`, turn `now` (chunk c+1, loaded an iteration ago) into
    // magnitudes in the ring half the consumer is not reading
    auto produce = [&](const int c, const float2 *now, float2 *nxt) {
        if (c + 1 >= nchunks) return;
        if (c + 2 < nchunks) tracker_load<PER_PROD>(kp, x0, stride, (c + 2) * TR_CH, pfirst, active, nxt);
        tracker_mag<PER_PROD, BINS>(now, pfirst, ring[(c + 1) & 1], col, raw);
    };
    // (probe builds: TR_PROBE_NO_CONSUME / TR_PROBE_NO_PRODUCE drop one role -- wrong results, the other role's time)
    // Round 4 experiment (TR_RAW_BARRIER 1): the chunk barriers order LDS traffic only (the ring), so they could be
    // `s_waitcnt lgkmcnt(0); s_barrier` instead of __syncthreads() -- a fence + barrier = `s_waitcnt vmcnt(0)` as well, which makes
    // every producer sit out the loads it has just issued for the chunk after next and the consumer the acknowledgement of its
    // 256-byte mask store.  Bit-identical masks, and no faster (see below): kept off.
#ifndef TR_RAW_BARRIER
#define TR_RAW_BARRIER 0 // measured: tracker 0.1736 -> 0.1747 ms (event pair), 0.096 -> 0.101 (prefix): no gain -- the chunk time is the consumer's
#endif                   // 64 dependent steps; the drains it skips were hidden behind them

    auto chunk_barrier = [&]() {
#if TR_RAW_BARRIER
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#else
        __syncthreads();
#endif
    };
    for (int c = 0; c < nchunks; c += 2) {
#ifndef TR_PROBE_NO_CONSUME
        if (w == 0) consume(c);
#endif
#ifndef TR_PROBE_NO_PRODUCE
        if (w != 0 && producer) produce(c, xa, xb);
#endif
        chunk_barrier();
        if (c + 1 < nchunks) {
#ifndef TR_PROBE_NO_CONSUME
            if (w == 0) consume(c + 1);
#endif
#ifndef TR_PROBE_NO_PRODUCE
            if (w != 0 && producer) produce(c + 1, xb, xa);
#endif
        }
        chunk_barrier();
    }
}

// ------------------------------------------------------------------------------------------------------------ K3
// Covariance + eigen-gate + eigenvector.  Only TF bins that pass the noise gate need the (float64, ~700 instruction)
// solve, and they are scattered: a wave that owns 64 fixed bins runs the solve if ANY lane is valid.  So each workgroup
// takes a tile of K3_FT frames x K3_NT (128) bins of one clip, compacts the valid (frame, bin) pairs into an LDS work list
// (lane order preserved, so neighbouring lanes still read neighbouring bins), writes zeros for the rest, and then the
// 256 lanes walk the dense list.  FEAT: write float32 channels 4-6 of the feature array (zeros above the DOA band up
// to F); otherwise write the float64 (3, n_bins, n_frames) array of extract_normalized_eigenvector (+ gate codes).
#ifndef K3_GROUP
#define K3_GROUP 2
#endif
constexpr int K3_OW = K3_NT + 8; // columns of the LDS output tile: a block's bins + the zero band above them when it fits
// Tile order.  Workgroups are dealt round-robin to the 8 XCDs (workgroup b runs on XCD b % 8, each with its own L2), so with
// tile = blockIdx.x two neighbouring 8-frame tiles -- which share 6 of the 14 spill frames they read -- always sit on
// different XCDs and the shared frames are fetched from HBM twice.  Runs of K3_XCD_CHUNK consecutive tiles are instead given to
// ONE XCD (the j-th workgroup of XCD x takes tile (j / CHUNK * 8 + x) * CHUNK + j % CHUNK): neighbours run on the same L2 at
// about the same time, while the runs themselves still rotate over the XCDs (bursts of heavy tiles spread over all eight).
#ifndef K3_XCD_CHUNK
#define K3_XCD_CHUNK 16
#endif

// FAST (round 3; tracking on, compile-time window): the work-list loop compiles ONLY the gate and the column-0 eigenvector
// (salsa_math.h, PATH 1); a gated bin whose column-0 pivot is too small (u_0 ~ 0: rare) is pushed onto a second LDS list and
// solved after the loop by the general arg-max path (PATH 2), one frame at a time.
//
// PK (round 4; FEAT + FAST, FOA / MIC, cond > 1): the two frames of a work item are solved TOGETHER as one packed-float32 pair
// (salsa_math.h: herm4_gate_eigvec_pk -- every v_pk_*_f32 does useful work in both halves), on covariances accumulated in float32
// in the (re, im) packing the spectra are loaded in (cov4pk_rank1: 16 packed FMAs per frame against 40 float64 instructions).
// A frame whose gate margin, pivot or feature conditioning is inside the float32 error bound comes back `unsure` and joins the
// float64 cold list, which recomputes its covariance in float64 from the spill (~1 % of the gated frames of the bench clips:
// tools/pk_study.py), so every gate decision the packed solve keeps equals the float64 one.
#ifndef K3_STAGE_LDS
#define K3_STAGE_LDS 0
#endif
#ifndef K3_OUT_NT
#define K3_OUT_NT 1
#endif
#ifndef K3_PK_WAVES
#define K3_PK_WAVES 4 // waves per SIMD the register allocation is held to (4: 128 VGPRs, 3: 168)
#endif
template <bool FEAT, int NHOP, bool FAST = false, bool PK = false>
__global__ __launch_bounds__(K3_NT, PK ? K3_PK_WAVES : 1) void cov_eig_kernel(const KParams kp, const float4 *__restrict__ Xs,
                                                      const unsigned *__restrict__ valid32,
                                                      float *__restrict__ out_feat, double *__restrict__ out_eig,
                                                      unsigned char *__restrict__ gate)
{
    constexpr int G = NHOP >= 0 ? K3_GROUP : 1; // frames per work item (compile-time window only)
    constexpr bool PAIRED = G > 1;
    static_assert(K3_FT % G == 0 && G <= 4 && K3_FT / G <= 16, "work-list entry layout");
    __shared__ unsigned short list[K3_FT * K3_NT];
    __shared__ unsigned short slow[FAST ? K3_FT * K3_NT : 1]; // (frame in tile) << 8 | bin in block
    __shared__ int count, nslow;
    // byte offsets (into the clip's spill) of frames t0 - NHOP .. t0 + K3_FT - 1 + NHOP with np.pad's 'wrap' on the time axis
    // (:43) applied, computed once per workgroup: done per lane and per frame in the work-list loop, the wrap compiled to an
    // integer-division sequence plus a loop, ~40 instructions x 8 frames per item -- a quarter of the loop's issue slots
    __shared__ __attribute__((aligned(16))) unsigned rowoff[NHOP >= 0 ? K3_FT + 2 * NHOP + 2 : 2];
    // FEAT: the tile's channels 4-6 are assembled in LDS (zeros + the gated bins' results) and written out as whole rows with
    // 16-byte stores at the end, instead of one 4-byte store per lane per (channel, frame) for the zeros plus three scattered
    // 4-byte stores per result
    __shared__ __attribute__((aligned(16))) float otile[FEAT ? 3 * K3_FT * K3_OW : 4];
#if K3_STAGE_LDS
    // Round-5 experiment (review item 6): the tile's 14 frames x 2 pairs x K3_NT bins copied into LDS with coalesced 16-byte loads
    // once per workgroup, the work items' sixteen gathers answered from there.  Measured slower (profiles/r5_ab_notes.txt): off.
    __shared__ __attribute__((aligned(16))) float4 stage[PK ? (K3_FT + 6) * 2 * K3_NT : 1];
#endif
    const int tid = threadIdx.x;
    const int Tn = kp.T;
    int tile = blockIdx.x, b = blockIdx.y;
    if (K3_XCD_CHUNK > 0) {
        const unsigned ntile = gridDim.x, total = ntile * gridDim.y, lin = blockIdx.x + ntile * blockIdx.y;
        constexpr unsigned span = 8u * (K3_XCD_CHUNK > 0 ? K3_XCD_CHUNK : 1);
        if (lin < total / span * span) { // (the ragged tail keeps the identity order)
            const unsigned xcd = lin & 7u, j = lin >> 3;
            const unsigned tl = ((j / (span / 8)) * 8u + xcd) * (span / 8) + j % (span / 8);
            b = (int)(tl / ntile);
            tile = (int)(tl - (unsigned)b * ntile);
        }
    }
    const int t0 = tile * K3_FT;
    const int nft = Tn - t0 < K3_FT ? Tn - t0 : K3_FT;
    const int bin0 = blockIdx.z * K3_NT;
    const int nbc = kp.nd - bin0 < K3_NT ? kp.nd - bin0 : K3_NT; // bins of this tile
    if (tid == 0) count = 0, nslow = 0;
    if (kp.doubt32 && tid < K3_FT * (K3_NT / 32)) { // this tile's words of the doubt mask (no other workgroup touches them): zero before any atomicOr below
        const int ft = tid % K3_FT, g32 = bin0 / 32 + tid / K3_FT, n32 = (kp.nd + TR_BINS - 1) / TR_BINS;
        if (ft < nft && g32 < n32) kp.doubt32[((long)b * n32 + g32) * Tn + t0 + ft] = 0u;
    }
    if (NHOP >= 0 && tid < K3_FT + 2 * NHOP) {
        int tt = t0 - NHOP + tid;
        while (tt < 0) tt += Tn;
        while (tt >= Tn) tt -= Tn;
        rowoff[tid] = (unsigned)tt * (16u * 2u * (unsigned)kp.nd);
    }
    if (FEAT) {
        for (int i = tid; i < 3 * K3_FT * K3_OW / 4; i += K3_NT) ((float4 *)otile)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    float *of = FEAT ? out_feat + ((long)b * kp.OC + 4) * Tn * kp.F : nullptr; // channels 4-6 of this clip, [3][T][F]
    double *oe = FEAT ? nullptr : out_eig + (long)b * 3 * kp.nd * Tn;
    unsigned char *og = (!FEAT && gate) ? gate + (long)b * kp.nd * Tn : nullptr;
    auto emit = [&](int t, int bin, const double *e, unsigned char g) {
        if (FEAT) {
#pragma unroll
            for (int i = 0; i < 3; i++) otile[(i * K3_FT + (t - t0)) * K3_OW + (bin - bin0)] = (float)e[i];
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) oe[((long)i * kp.nd + bin) * Tn + t] = e[i];
            if (og) og[(long)bin * Tn + t] = g;
        }
    };
    const double zero3[3] = {0.0, 0.0, 0.0};
    {
        // Compaction.  lane = bin; a wave covers exactly one 64-bin group, so the gate mask of (frame, group) -- one ballot
        // over the lanes' history bits -- is a wave-uniform scalar whose bits ARE the lanes to keep.  Each wave counts its
        // K3_FT masks with scalar popcounts, reserves its slice of the work list with ONE LDS atomic, and every kept lane
        // drops its (frame, bin) at slice + (bits below it): lane order survives, so neighbouring list entries are
        // neighbouring bins.
        const int bl = tid;
        const bool in = bl < nbc;
        const int ng32 = (kp.nd + TR_BINS - 1) / TR_BINS;
        const int bin = bin0 + bl;
        const int lane = tid & 63;
        const int grp = __builtin_amdgcn_readfirstlane(bin >> 6); // the wave's 64-bin group = two of the tracker's 32-bin groups
        const unsigned long long inmask = __ballot(in);
        // the tracker's per-frame masks of this wave's bins (two 32-bin groups x K3_FT frames): ONE vector load -- lane l takes
        // frame l % K3_FT of half l / K3_FT -- then readlane; the masks are wave-uniform scalars and no ballot is needed.
        // (Scalar loads here were measured 40 % slower for the whole kernel: sixteen serialised scalar-cache misses per wave.)
        static_assert(2 * K3_FT <= 64, "one lane per (half, frame)");
        unsigned myw = 0u;
        if (kp.tracking && lane < 2 * K3_FT) {
            const int ft = lane % K3_FT, half = lane / K3_FT;
            if (ft < nft && 2 * grp + half < ng32) myw = valid32[((long)b * ng32 + 2 * grp + half) * Tn + t0 + ft];
        }
        unsigned long long words[K3_FT];
        int total = 0;
#pragma unroll
        for (int ft = 0; ft < K3_FT; ft++) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)myw, ft), hi = (unsigned)__builtin_amdgcn_readlane((int)myw, K3_FT + ft);
            const unsigned long long tr = (((unsigned long long)hi << 32) | lo) & inmask;
            words[ft] = kp.tracking ? tr : (ft < nft ? inmask : 0ull);
        }
        // A work item is a GROUP of G neighbouring frames of one bin with at least one of them gated in.
        auto any_of = [&](int ft) {
            unsigned long long wd = 0ull;
#pragma unroll
            for (int j = 0; j < G; j++) wd |= words[ft + j];
            return wd;
        };
#pragma unroll
        for (int ft = 0; ft < K3_FT; ft += G) total += __popcll(any_of(ft));
        int base = 0;
        if (lane == 0 && total) base = atomicAdd(&count, total);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int ft = 0; ft < K3_FT; ft += G) {
            const unsigned long long wd = any_of(ft);
            if (in) {
                unsigned v = 0; // which frames of the group are gated in
#pragma unroll
                for (int j = 0; j < G; j++) v |= ((unsigned)(words[ft + j] >> lane) & 1u) << j;
                if (v) list[base + __popcll(wd & ((1ull << lane) - 1))] = (unsigned short)((v << 12) | ((ft / G) << 8) | bl);
#pragma unroll
                for (int j = 0; j < G; j++)
                    if (!FEAT && ft + j < nft && !((v >> j) & 1)) emit(t0 + ft + j, bin, zero3, 0);
            }
            base += __popcll(wd);
        }
    }
    // columns of this block's rows: its bins, plus -- in the last block -- the zeros above the DOA band up to F (:373-374)
    const int seg = (FEAT && blockIdx.z == gridDim.z - 1) ? (kp.F - bin0 < K3_OW ? kp.F - bin0 : K3_OW) : nbc;
    if (FEAT && blockIdx.z == gridDim.z - 1 && kp.F - bin0 > K3_OW) { // (wider than the LDS tile: the rest directly)
        const int first = bin0 + K3_OW, tail = kp.F - first;
        for (int i = tid; i < nft * tail; i += K3_NT) {
            const int ft = i / tail, f = first + (i - ft * tail);
#pragma unroll
            for (int c = 0; c < 3; c++) st_off(of, 4u * (unsigned)((c * Tn + t0 + ft) * kp.F + f), 0.f);
        }
    }
    __syncthreads();
    const int n = count;
    const int stride = 2 * kp.nd;
    const int nhop = NHOP >= 0 ? NHOP : kp.n_hop;
    const float4 *xclip = Xs + (long)b * Tn * stride;
    // :111-112 the coherence test only gates when tracking -- except in contrib, whose test always gates (:352-354)
    const bool ungated = !kp.tracking && !kp.flex;
    auto solve_emit = [&](const salsa::herm4<double> &R, int t, int bin, auto path) {
        constexpr int PATH = decltype(path)::value;
        const bool foa = kp.format == SALSA_FORMAT_FOA;
        const salsa::eig_result<double> er = salsa::herm4_gate_eigvec<PATH>(R, kp.cond, kp.inv_cond, ungated, !foa);
        if (PATH == 1 && er.fallback) { // passed the gate, pivot too small: the cold loop below takes it
            slow[atomicAdd(&nslow, 1)] = (unsigned short)(((t - t0) << 8) | (bin - bin0));
            return;
        }
        if (er.doubt && kp.doubt32 && !ungated) { // the threshold sits ON a root of the quartic: what is emitted below is provisional,
            atomicOr(&kp.doubt32[((long)b * ((kp.nd + TR_BINS - 1) / TR_BINS) + (bin >> 5)) * Tn + t], 1u << (bin & 31)); // gate_doubt_kernel decides
            atomicOr(kp.doubt_flag, 1u);
        }
        double e[3] = {0.0, 0.0, 0.0};
        unsigned char g = er.rank1 ? 2 : 1;
        if (er.rank1 || ungated) {
            const int k = bin + kp.lower;
            // delta*k (:121-123); contrib divides by a float32 frequency vector with [0] = 1 (:188-190)
            const double den = kp.flex ? (double)((float)(k == 0 ? 1 : k) * (float)kp.delta) : kp.delta * (double)k;
            if (PATH != 2 && er.col0) { // gated fast path: column 0 of the adjugate, real pivot (salsa_math.h)
                if (foa) salsa::normalise_foa_col0(er.u, e);
                else salsa::normalise_mic_col0(er.u, den, e);
            } else if (PATH != 1) {
                if (foa) salsa::normalise_foa(er.u, e, ungated);
                else salsa::normalise_mic(er.u, den, e);
            }
            g = 2;
        } else if (FEAT && kp.flex && !kp.tracking) {
            e[0] = __builtin_nan(""); // marks "failed the test" for flex_allpass_kernel (a passing bin can be exactly 0)
        }
        emit(t, bin, e, g);
    };
    using hot_path = std::integral_constant<int, FAST ? 1 : 2>;
    using cold_path = std::integral_constant<int, 2>;
    if constexpr (PK) {
        static_assert(!PK || (G == 2 && FEAT && FAST && NHOP >= 0), "the packed solve takes the two frames of a pair");
        // Float32 all the way.  (Tried and dropped: issuing the NEXT item's sixteen gathers between this item's covariance and
        // its solve.  The solve needs ~130 registers by itself, so the prefetched 64 push the loop to 195 VGPRs -- 2 waves per
        // SIMD -- or, held to 128 / 168, into scratch: 0.50 - 0.88 ms against 0.38, profiles/r4_k3_pk_ab.txt.)
        constexpr int NW = 2 * NHOP + 2;
        const unsigned half = 16u * (unsigned)kp.nd;
#if K3_STAGE_LDS
        if (n > 0) { // (a tile with nothing gated stages nothing)
            for (int i = tid; i < (K3_FT + 6) * 2 * K3_NT; i += K3_NT) {
                const int fr = i / (2 * K3_NT), rem = i - fr * 2 * K3_NT, pr = rem / K3_NT, bl = rem - pr * K3_NT;
                if (bl < nbc) stage[i] = ld_off(xclip, rowoff[fr] + 16u * (unsigned)(bin0 + bl) + (pr ? half : 0u));
            }
        }
        __syncthreads();
#endif
        for (int s = tid; s < n; s += K3_NT) {
            const int i = list[s];
            const int ft = 2 * ((i >> 8) & 15), bl = i & 255; // entry = validity of the pair's frames << 12 | pair << 8 | bin
            float4 xa[NW], xc[NW];
            {
                const unsigned *ro = rowoff + ft; // frames t - NHOP .. t + 1 + NHOP (np.pad(..., 'wrap') on the time axis, :43)
                const unsigned boff = 16u * (unsigned)(bin0 + bl);
#pragma unroll
                for (int k = 0; k < NW; k++) {
#if K3_STAGE_LDS
                    xa[k] = stage[((ft + k) * 2 + 0) * K3_NT + bl];
                    xc[k] = stage[((ft + k) * 2 + 1) * K3_NT + bl];
                    (void)ro; (void)boff;
#else
                    const unsigned r = ro[k];
                    xa[k] = K3_GATHER_NT ? ld_off_nt(xclip, r + boff) : ld_off(xclip, r + boff);
                    xc[k] = K3_GATHER_NT ? ld_off_nt(xclip, r + boff + half) : ld_off(xclip, r + boff + half);
#endif
                }
            }
            auto chans = [&](int k, salsa::pk2f *v) {
                v[0] = salsa::pk2f{xa[k].x, xa[k].y};
                v[1] = salsa::pk2f{xa[k].z, xa[k].w};
                v[2] = salsa::pk2f{xc[k].x, xc[k].y};
                v[3] = salsa::pk2f{xc[k].z, xc[k].w};
            };
            // the (re, im)-packed covariance of the six shared frames, one more frame for each window (both windows, also when
            // only one frame is gated in: the other half of every packed instruction is free)
            salsa::cov4pk Cc = {}, C0, C1;
            salsa::pk2f v[4];
#pragma unroll
            for (int k = 1; k <= 2 * NHOP; k++) {
                chans(k, v);
                salsa::cov4pk_rank1(Cc, Cc, v);
            }
            chans(0, v);
            salsa::cov4pk_rank1(C0, Cc, v);
            chans(2 * NHOP + 1, v);
            salsa::cov4pk_rank1(C1, Cc, v);
            const int live = (i >> 12) & 3;
            int odd;
            const salsa::herm4<salsa::pk2f> A = salsa::herm4_pk_from_windows(C0, C1, odd);
            salsa::pk2f e[3];
            salsa::pk_eig r;
            if (kp.format == SALSA_FORMAT_FOA) {
                r = salsa::herm4_gate_eigvec_pk<false>(A, (float)kp.cond, (float)kp.inv_cond, live & ~odd);
                if (r.pass) salsa::normalise_foa_pk(r, e);
            } else {
                r = salsa::herm4_gate_eigvec_pk<true>(A, (float)kp.cond, (float)kp.inv_cond, live & ~odd);
                if (r.pass) salsa::normalise_mic_pk(r, (float)(kp.delta * (double)(bin0 + bl + kp.lower)), e);
            }
            r.unsure |= odd & live;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if ((r.unsure >> j) & 1) // float64 decides: the cold loop below
                    slow[atomicAdd(&nslow, 1)] = (unsigned short)(((ft + j) << 8) | bl);
                else if ((r.pass >> j) & 1) {
#pragma unroll
                    for (int q = 0; q < 3; q++) otile[(q * K3_FT + ft + j) * K3_OW + bl] = e[q][j];
                }
            }
        }
    }
    for (int s = tid; !PK && s < n; s += K3_NT) {
        const int i = list[s];
        const int t = t0 + G * ((i >> 8) & 15); // entry = validity of the group's frames << 12 | group << 8 | bin
        const int bin = bin0 + (i & 255);
        const float4 *xb = xclip + bin;
        const unsigned row = 16u * (unsigned)stride, boff = 16u * (unsigned)bin, half = 16u * (unsigned)kp.nd; // bytes
        if (PAIRED) {
            // frames t-NHOP .. t+1+NHOP as independent 16-B loads issued together: the two windows share 2*NHOP frames, so a
            // pair costs 2*NHOP+2 gathers instead of 2*(2*NHOP+1) (the gate mask is bursty in time: 1.8 of 2 frames of a
            // listed pair are gated in on the bench clips).  Splitting the loads into batches to save VGPRs was measured
            // slower: their latency is what this kernel hides.
            constexpr int NW = NHOP >= 0 ? 2 * NHOP + G : G;
            float4 xa[NW], xc[NW];
            const unsigned *ro = rowoff + (t - t0); // frames t - NHOP .. (np.pad(..., 'wrap') on the time axis, :43: the table)
#pragma unroll
            for (int k = 0; k < NW; k++) {
                const unsigned r = ro[k];
                xa[k] = ld_off(xclip, r + boff);
                xc[k] = ld_off(xclip, r + boff + half);
            }
            auto frame = [&](int k, salsa::herm4<double> &A) {
                const cplx<double> x[4] = {{(double)xa[k].x, (double)xa[k].y}, {(double)xa[k].z, (double)xa[k].w},
                                           {(double)xc[k].x, (double)xc[k].y}, {(double)xc[k].z, (double)xc[k].w}};
                salsa::herm4_rank1_add(A, x);
            };
            salsa::herm4<double> Rc = {}; // the frames every window of the group contains
#pragma unroll
            for (int k = G - 1; k <= 2 * NHOP; k++) frame(k, Rc);
#pragma unroll
            for (int j = 0; j < G; j++) {
                if ((i >> (12 + j)) & 1) {
                    salsa::herm4<double> R = Rc;
#pragma unroll
                    for (int k = j; k < G - 1; k++) frame(k, R);
#pragma unroll
                    for (int k = 2 * NHOP + 1; k <= 2 * NHOP + j; k++) frame(k, R);
                    solve_emit(R, t + j, bin, hot_path{});
                }
            }
        } else {
            salsa::herm4<double> R = {};
            for (int k = -nhop; k <= nhop; k++) {
                int tt = t + k;
                while (tt < 0) tt += Tn;
                while (tt >= Tn) tt -= Tn;
                const float4 a = xb[tt * stride], c = xb[tt * stride + kp.nd];
                const cplx<double> x[4] = {{(double)a.x, (double)a.y}, {(double)a.z, (double)a.w},
                                           {(double)c.x, (double)c.y}, {(double)c.z, (double)c.w}};
                salsa::herm4_rank1_add(R, x);
            }
            solve_emit(R, t, bin, hot_path{});
        }
    }
    if (FAST) { // cold loop: the few gated bins the hot loop could not finish, general path, one frame per item
        __syncthreads();
        const int ns = nslow;
        if (kp.stats && tid == 0) { // (verification counters; NULL in production)
            int live = 0;
            for (int s = 0; s < n; s++) live += __popc((list[s] >> 12) & 15);
            atomicAdd(&kp.stats[0], (unsigned long long)n);
            atomicAdd(&kp.stats[1], (unsigned long long)live);
            atomicAdd(&kp.stats[2], (unsigned long long)ns);
            atomicAdd(&kp.stats[3], 1ull);
        }
        for (int s = tid; s < ns; s += K3_NT) {
            const int i = slow[s];
            const int t = t0 + (i >> 8), bin = bin0 + (i & 255);
            const float4 *xb = xclip + bin;
            salsa::herm4<double> R = {};
            for (int k = -nhop; k <= nhop; k++) {
                int tt = t + k;
                while (tt < 0) tt += Tn;
                while (tt >= Tn) tt -= Tn;
                const float4 a = xb[tt * stride], c = xb[tt * stride + kp.nd];
                const cplx<double> x[4] = {{(double)a.x, (double)a.y}, {(double)a.z, (double)a.w},
                                           {(double)c.x, (double)c.y}, {(double)c.z, (double)c.w}};
                salsa::herm4_rank1_add(R, x);
            }
            solve_emit(R, t, bin, cold_path{});
        }
    }
    if (FEAT) { // write the tile out: 3 channels x nft frames, `seg` consecutive floats each
        __syncthreads();
        const bool vec = !(kp.F & 3) && !(seg & 3) && !(bin0 & 3); // rows start and end on 16-byte boundaries
        if (vec) {
            const int q = seg >> 2;
            for (int i = tid; i < 3 * nft * q; i += K3_NT) {
                const int row = i / q, col = i - row * q, c = row / nft, ft = row - c * nft;
                float4 *dst = (float4 *)(of + ((long)(c * Tn + t0 + ft) * kp.F + bin0 + 4 * col));
                const float4 val = *(const float4 *)(otile + (c * K3_FT + ft) * K3_OW + 4 * col);
                if (K3_OUT_NT) st_off_nt(dst, 0u, val); // (production default since round 5: rows written once, never re-read by this kernel)
                else *dst = val;
            }
        } else {
            for (int i = tid; i < 3 * nft * seg; i += K3_NT) {
                const int row = i / seg, col = i - row * seg, c = row / nft, ft = row - c * nft;
                of[(long)(c * Tn + t0 + ft) * kp.F + bin0 + col] = otile[(c * K3_FT + ft) * K3_OW + col];
            }
        }
    }
}

// The TF bins cov_eig_kernel flagged in kp.doubt32 -- the threshold mu1 / cond numerically ON a root of the characteristic quartic, which
// then cannot decide "s0 > s1 * cond" (:106): multiple eigenvalues at the threshold lose float64 to sqrt / cube-root precision -- decided
// on the matrix: float64 covariance from the spill, eigenvalues by Jacobi rotations (salsa_math.h herm4_rank1_by_jacobi, the oracle's
// method), eigenvector by the general adjugate path, and the bin's three values rewritten.  On natural signals nothing is flagged:
// the launch (64 workgroups) reads the group's flag word and exits; only a flagged launch scans the mask.  Round 6.
template <bool FEAT>
__global__ __launch_bounds__(256) void gate_doubt_kernel(const KParams kp, const float4 *__restrict__ Xs, float *__restrict__ out_feat,
                                                         double *__restrict__ out_eig, unsigned char *__restrict__ gate)
{
    if (*(const volatile unsigned *)kp.doubt_flag == 0u) return; // nothing flagged (every natural signal): one load per wave
    const int Tn = kp.T, n32 = (kp.nd + TR_BINS - 1) / TR_BINS, stride = 2 * kp.nd;
    const long nwords = (long)kp.B * n32 * Tn;
    const bool foa = kp.format == SALSA_FORMAT_FOA;
    for (long wi = (long)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords; wi += (long)gridDim.x * blockDim.x) {
        unsigned word = kp.doubt32[wi];
        if (!word) continue;
        const int t = (int)(wi % Tn), g32 = (int)((wi / Tn) % n32), b = (int)(wi / ((long)Tn * n32));
        while (word) {
            const int j = __ffs((int)word) - 1;
            word &= word - 1u;
            const int bin = 32 * g32 + j;
            const float4 *xb = Xs + (long)b * Tn * stride + bin;
            salsa::herm4<double> R = {};
            for (int k = -kp.n_hop; k <= kp.n_hop; k++) { // the cold loop's covariance, term for term
                int tt = t + k;
                while (tt < 0) tt += Tn;
                while (tt >= Tn) tt -= Tn;
                const float4 a = xb[tt * stride], c = xb[tt * stride + kp.nd];
                const cplx<double> x[4] = {{(double)a.x, (double)a.y}, {(double)a.z, (double)a.w},
                                           {(double)c.x, (double)c.y}, {(double)c.z, (double)c.w}};
                salsa::herm4_rank1_add(R, x);
            }
            const bool rank1 = salsa::herm4_rank1_by_jacobi(R, kp.cond);
            double e[3] = {0.0, 0.0, 0.0};
            if (rank1) {
                const salsa::eig_result<double> er = salsa::herm4_gate_eigvec<2>(R, kp.cond, kp.inv_cond, true, !foa);
                const int k = bin + kp.lower;
                const double den = kp.flex ? (double)((float)(k == 0 ? 1 : k) * (float)kp.delta) : kp.delta * (double)k;
                if (foa) salsa::normalise_foa(er.u, e, false);
                else salsa::normalise_mic(er.u, den, e);
            } else if (FEAT && kp.flex && !kp.tracking) {
                e[0] = __builtin_nan(""); // "failed the test" for flex_allpass_kernel, as cov_eig_kernel marks it
            }
            if (FEAT) {
#pragma unroll
                for (int i = 0; i < 3; i++) out_feat[(((long)b * kp.OC + 4 + i) * Tn + t) * kp.F + bin] = (float)e[i];
            } else {
#pragma unroll
                for (int i = 0; i < 3; i++) out_eig[(((long)b * 3 + i) * kp.nd + bin) * Tn + t] = e[i];
                if (gate) gate[((long)b * kp.nd + bin) * Tn + t] = rank1 ? 2 : 1;
            }
        }
    }
}

// contrib/salsa_flexible.py with is_tracking=False: ONE all-pass mask array is created (:336-337) and then narrowed in
// place by "mask[mask] = good_coherence_mask" (:354), so a bin that fails the coherence test once is never looked at
// again in that clip.  cov_eig_kernel marks failures with NaN in channel 4; this pass (lane = bin, coalesced rows,
// sequential in time) zeroes everything from a bin's first failure on.
__global__ __launch_bounds__(256) void flex_allpass_kernel(const KParams kp, float *__restrict__ out)
{
    const int bin = blockIdx.x * 256 + threadIdx.x;
    if (bin >= kp.nd) return;
    float *of = out + ((long)blockIdx.y * kp.OC + kp.nch) * kp.T * kp.F + bin; // first spatial plane
    bool dead = false;
    for (int t = 0; t < kp.T; t++) {
        const float v = of[t * kp.F];
        dead = dead || (v != v);
        if (dead) {
            for (int c = 0; c < kp.nch - 1; c++) of[(c * kp.T + t) * kp.F] = 0.f;
        }
    }
}

} // namespace

namespace salsa_impl {

void launch_tracker(const KParams &kp, hipStream_t s, const float4 *Xs, unsigned *valid32)
{
    hipLaunchKernelGGL(tracker_kernel, dim3(tracker_grid(kp)), dim3(64 * TR_WAVES), 0, s, kp, Xs, valid32);
}

template <bool FEAT>
static void launch_gate_doubt(const KParams &kp, hipStream_t s, const float4 *Xs, float *out_feat, double *out_eig, unsigned char *gate)
{
    if (!kp.doubt32) return;
    const long nwords = (long)kp.B * ((kp.nd + TR_BINS - 1) / TR_BINS) * kp.T;
    const unsigned blocks = (unsigned)(nwords < 256L * 64 ? (nwords + 255) / 256 : 64);
    hipLaunchKernelGGL(gate_doubt_kernel<FEAT>, dim3(blocks ? blocks : 1u), dim3(256), 0, s, kp, Xs, out_feat, out_eig, gate);
}

template <bool FEAT>
void launch_cov_eig(const KParams &kp, dim3 grid, hipStream_t s, const float4 *Xs, const unsigned *valid,
                    float *out_feat, double *out_eig, unsigned char *gate)
{
    const bool gated = kp.tracking || kp.flex; // (!ungated: the coherence test decides, so passing bins have a spectral gap)
    if (kp.doubt32 && !kp.tracking) (void)hipMemsetAsync(kp.doubt_flag, 0, sizeof(unsigned), s); // (no tracker launch zeroed it: contrib's gate without tracking)
    // (the packed pair solve: feature output only -- salsa_eigvec_batch keeps float64 results -- and never for contrib's variant)
    if (FEAT && SALSA_PK && K3_GROUP == 2 && kp.n_hop == 3 && gated && SALSA_COL0 && !kp.flex && kp.cond >= SALSA_PK_COND_MIN && kp.cond < 1e6 && !kp.force_f64)
        hipLaunchKernelGGL((cov_eig_kernel<FEAT, 3, true, FEAT && K3_GROUP == 2>), grid, dim3(K3_NT), 0, s, kp, Xs, valid, out_feat, out_eig, gate);
    else if (kp.n_hop == 3 && gated && SALSA_COL0)
        hipLaunchKernelGGL((cov_eig_kernel<FEAT, 3, true>), grid, dim3(K3_NT), 0, s, kp, Xs, valid, out_feat, out_eig, gate);
    else if (kp.n_hop == 3)
        hipLaunchKernelGGL((cov_eig_kernel<FEAT, 3>), grid, dim3(K3_NT), 0, s, kp, Xs, valid, out_feat, out_eig, gate);
    else
        hipLaunchKernelGGL((cov_eig_kernel<FEAT, -1>), grid, dim3(K3_NT), 0, s, kp, Xs, valid, out_feat, out_eig, gate);
    launch_gate_doubt<FEAT>(kp, s, Xs, out_feat, out_eig, gate); // (a no-op unless kp.doubt32: gated plans)
}

template void launch_cov_eig<true>(const KParams &, dim3, hipStream_t, const float4 *, const unsigned *, float *, double *, unsigned char *);
template void launch_cov_eig<false>(const KParams &, dim3, hipStream_t, const float4 *, const unsigned *, float *, double *, unsigned char *);

void launch_flex_allpass(const KParams &kp, hipStream_t s, float *out)
{
    hipLaunchKernelGGL(flex_allpass_kernel, dim3((unsigned)((kp.nd + 255) / 256), (unsigned)kp.B), dim3(256), 0, s, kp, out);
}

// one K1 launch with the window `win` (one of the plan's two tables)
int launch_stft(salsa_plan *pl, const KParams &kp, const double *win, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s)
{
    const bool lite = kp.feature == SALSA_FEATURE_LITE || kp.feature == SALSA_FEATURE_IPD;
    const bool single = !lite && kp.pair_sel >= 0; // one channel pair per launch: twice the frames per wave, same work per wave
    constexpr int NF_FULL = k1_cfg<false>::NF, NF_LITE = k1_cfg<true>::NF, NF_PAIR = 2 * k1_cfg<false>::NF;
    const int fpb = 4 * (lite ? NF_LITE : single ? NF_PAIR : NF_FULL); // frames per workgroup
    const unsigned nblk = (unsigned)((kp.T + fpb - 1) / fpb);
    dim3 grid(nblk, (unsigned)kp.B);
    // a scaler is attached: the instantiation with the tables in LDS -- which hold [2][4 * 256] floats, so only while F <= 256 (the
    // contrib plan with SALSA_FLAG_NO_CLIP_FREQS and a lite band from bin 0 have F = 257: they take the plain kernel, whose
    // store path reads the tables from global memory at any F)
    // the dataset scripts' layout as a compile-time fact (stft_kernel's STD instantiations; K1_STD 0: the general kernel, for A/B)
    // (STD instantiations: plans with one window only -- a SALSA plan with win_len < n_fft takes the general kernel, twice)
    const bool one_window = pl->d_window == pl->d_window_doa;
    const bool std_layout = K1_STD && one_window && pl->p.n_fft == 512 && !lite && !single && kp.feature == SALSA_FEATURE_SALSA && kp.compress &&
                            kp.spec_lo == 1 && kp.spec_hi == 193 && kp.ident == 192 && kp.F == 200 && kp.nch == 4 &&
                            kp.layout == SALSA_LAYOUT_PLANAR && kp.pair_sel < 0;
    const bool lite_std = K1_LITE_STD && one_window && pl->p.n_fft == 512 && lite && kp.nch == 4 && kp.layout == SALSA_LAYOUT_PLANAR && !kp.sc_mean &&
                          kp.cutoff <= 256 && kp.pair_sel < 0;
    if (lite_std) {
        hipLaunchKernelGGL((stft_kernel<512, double, true, NF_LITE, 2, false, true>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    } else if (std_layout) {
        constexpr size_t SCT_BYTES = 2 * 4 * 256 * sizeof(float);
        if (kp.sc_mean) hipLaunchKernelGGL((stft_kernel<512, double, false, NF_FULL, 2, true, true>), grid, dim3(256), SCT_BYTES, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<512, double, false, NF_FULL, 2, false, true>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    } else if (pl->p.n_fft == 1024) {
        // SALSA-Lite / IPD only (salsa_plan_create).  One instantiation for every layout; an attached scaler is read from global memory
        // in the store path (F = 382 at the defaults: the LDS tables of the SC instantiations hold 256 bins)
        if (!lite) return fail(SALSA_ENFFT, "n_fft 1024 is a SALSA-Lite / SALSA-IPD size%s");
        hipLaunchKernelGGL((stft_kernel<1024, double, true, NF_LITE>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    } else if (pl->p.n_fft == 512 && kp.sc_mean && !single && kp.F <= 256) {
        constexpr size_t SCT_BYTES = 2 * 4 * 256 * sizeof(float);
        if (lite) hipLaunchKernelGGL((stft_kernel<512, double, true, NF_LITE, 2, true>), grid, dim3(256), SCT_BYTES, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<512, double, false, NF_FULL, 2, true>), grid, dim3(256), SCT_BYTES, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    } else if (pl->p.n_fft == 512) {
        if (lite) hipLaunchKernelGGL((stft_kernel<512, double, true, NF_LITE>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else if (single) hipLaunchKernelGGL((stft_kernel<512, double, false, NF_PAIR>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<512, double, false, NF_FULL>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    } else {
        if (lite) hipLaunchKernelGGL((stft_kernel<256, double, true, NF_LITE>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else if (single) hipLaunchKernelGGL((stft_kernel<256, double, false, NF_PAIR>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<256, double, false, NF_FULL>), grid, dim3(256), 0, s, kp, d_audio, win, pl->d_tw, d_out, Xs);
    }
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

// K1 of salsa_extract_batch.  One window: one launch.  Full SALSA with win_len < n_fft: the spill (DOA spectra) comes from the
// n_fft window and the log-spectrogram channels from the win_len window, so the general kernel runs twice: with the DOA window
// (spill + provisional channels 0-3), then log-spec only (no spill store) with the spectrogram window, overwriting channels 0-3 of
// the 7-channel output (fused scaler included).  Same stream: the second launch's stores land last.
int launch_k1(salsa_plan *pl, const KParams &kp, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s)
{
    if (pl->d_window == pl->d_window_doa || kp.feature != SALSA_FEATURE_SALSA) return launch_stft(pl, kp, pl->d_window, d_audio, d_out, Xs, s);
    const int rc = launch_stft(pl, kp, pl->d_window_doa, d_audio, d_out, Xs, s);
    if (rc) return rc;
    KParams lp = kp;
    lp.feature = FEATURE_LOGSPEC_ONLY; // (OC stays 7)
    return launch_stft(pl, lp, pl->d_window, d_audio, d_out, nullptr, s);
}

// K1 of salsa_extract_multichannel: NPAIRS channel pairs per clip (0: the count at run time, kp.nch / 2)
template <int NPAIRS>
int launch_stft_multi(salsa_plan *pl, const KParams &kp, const float *d_audio, float *d_out, float4 *Xs, hipStream_t s)
{
    const bool lite = kp.feature == SALSA_FEATURE_LITE;
    constexpr int NF = 4;
    dim3 grid((unsigned)((kp.T + 4 * NF - 1) / (4 * NF)), (unsigned)kp.B);
    if (pl->p.n_fft == 512) {
        if (lite) hipLaunchKernelGGL((stft_kernel<512, double, true, NF, NPAIRS>), grid, dim3(256), 0, s, kp, d_audio, pl->d_window, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<512, double, false, NF, NPAIRS>), grid, dim3(256), 0, s, kp, d_audio, pl->d_window, pl->d_tw, d_out, Xs);
    } else {
        if (lite) hipLaunchKernelGGL((stft_kernel<256, double, true, NF, NPAIRS>), grid, dim3(256), 0, s, kp, d_audio, pl->d_window, pl->d_tw, d_out, Xs);
        else hipLaunchKernelGGL((stft_kernel<256, double, false, NF, NPAIRS>), grid, dim3(256), 0, s, kp, d_audio, pl->d_window, pl->d_tw, d_out, Xs);
    }
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}
template int launch_stft_multi<3>(salsa_plan *, const KParams &, const float *, float *, float4 *, hipStream_t);
template int launch_stft_multi<4>(salsa_plan *, const KParams &, const float *, float *, float4 *, hipStream_t);
template int launch_stft_multi<0>(salsa_plan *, const KParams &, const float *, float *, float4 *, hipStream_t);

} // namespace salsa_impl
