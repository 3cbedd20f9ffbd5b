// salsa_plan.hip -- the host side of the feature extractor's C ABI (include/salsa_hip.h): struct salsa_plan (salsa_internal.h)
// created, configured and destroyed; the workspace queries (the layout itself: salsa_workspace.h); timing marks; and the schedules of
// salsa_extract_batch as named steps -- issue_group (one group's launches, plain in-order issue when it is the whole batch),
// issue_forked (clip groups and split channel pairs on the plan's streams), replay_graph (the captured hipGraph) -- with
// salsa_logspec_batch and the two salsa_eigvec entry points.  Host code only: no kernel lives here, every launch goes through a launcher of salsa_internal.h
// (K1 / K2 / K3: salsa_kernels.hip; the fused kernel: fused_kernel.hip; relayout: multichannel.hip).
// The library's one error message is defined here: salsa_last_error / salsa_set_last_error_.
#include "build_guard.h" // probe switches need -DSALSA_PROBE_BUILD; SALSA_BUILD_FLAGS (generated: tools/gen_build_guard.py)
#include "salsa_internal.h"
#include <string.h>
#include <memory>
#include <vector>

using salsa::cplx;
using namespace salsa_impl;

namespace {

thread_local char g_err[512] = "";
constexpr double PI = 3.14159265358979323846;

} // namespace

namespace salsa_impl {

KParams make_kparams(const salsa_plan *pl, int batch, int64_t n_samples)
{
    KParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.B = batch;
    kp.N = (int)n_samples;
    kp.T = (int)(1 + n_samples / pl->p.hop_len);
    kp.hop = pl->p.hop_len;
    kp.lower = pl->lower;
    kp.upper = pl->upper;
    kp.nd = pl->nd;
    kp.cutoff = pl->cutoff;
    kp.F = pl->F;
    kp.OC = 7;
    kp.ident = pl->ident;
    kp.spec_lo = pl->spec_lo;
    kp.spec_hi = pl->spec_hi;
    kp.flex = pl->flex;
    kp.snr_ratio = pl->snr_ratio;
    kp.compress = pl->flex ? 0 : pl->p.is_compress_high_freq;
    kp.layout = pl->p.audio_layout;
    kp.feature = pl->p.feature_type;
    kp.format = pl->p.audio_format;
    kp.tracking = pl->p.is_tracking;
    kp.n_hop = pl->p.n_hopframes;
    kp.pair_sel = -1;
    kp.nch = 4;
    kp.cond = pl->p.cond_num;
    kp.inv_cond = pl->p.cond_num > 0 ? 1.0 / pl->p.cond_num : 0.0;
    kp.delta = pl->delta;
    kp.sc_mean = pl->sc_mean;
    kp.sc_std = pl->sc_std;
    kp.stats = pl->stats;
    kp.force_f64 = (pl->p.flags & SALSA_FLAG_FORCE_F64) != 0;
    return kp;
}

} // namespace salsa_impl

namespace {

// timing mode: bracket one launch with events on ITS stream
static int mark_begin(salsa_plan *pl, hipStream_t s, const char *name)
{
    if (!pl->timing || pl->n_kernels >= SALSA_MAX_KERNELS) return -1;
    const int i = pl->n_kernels++;
    pl->names[i] = name;
    if (!pl->ev0[i]) (void)hipEventCreate(&pl->ev0[i]);
    if (!pl->ev1[i]) (void)hipEventCreate(&pl->ev1[i]);
    (void)hipEventRecord(pl->ev0[i], s);
    return i;
}
static void mark_end(salsa_plan *pl, hipStream_t s, int i)
{
    if (i >= 0) (void)hipEventRecord(pl->ev1[i], s);
}

// One kernel of a schedule = ONE event pair in timing mode, whatever is launched between the pair.  With a repeat count
// (salsa_plan_set_timing(plan, K > 1)) a kernel that is idempotent on (audio, spill, masks) -- REPEATABLE -- is launched K times back
// to back between that pair, so the per-launch figure is elapsed / K with no event between the launches (an event pair around a
// single launch adds ~12 % to it); anything else is launched ONCE.  `launch` returns a SALSA code; the first failure ends the repeats.
enum Repeat { ONCE, REPEATABLE };
template <typename Launch>
static int timed(salsa_plan *pl, hipStream_t s, const char *name, Repeat repeat, Launch launch)
{
    const int reps = repeat == REPEATABLE && pl->timing > 1 ? pl->timing : 1;
    const int m = mark_begin(pl, s, name);
    int rc = SALSA_OK;
    for (int r = 0; r < reps && !rc; r++) rc = launch();
    mark_end(pl, s, m);
    return rc;
}

// one salsa_extract_batch call, as every step of its schedules sees it
struct ExtractCall {
    salsa_plan *pl;
    KParams kp;          // the whole batch (no workspace pointer bound: a group binds its own)
    const float *audio;
    float *out;
    bool full;           // full SALSA: the path goes on past K1, through the workspace
    void *ws;
    WorkspaceLayout lay;
    bool doubt;          // the plan gates: the doubt mask is bound
};

// The launches of group g = clips [g0, g1): every buffer is clip-major, so a group is just a pointer offset.  s1 runs the STFT
// launch(es); s2 the tracker and the covariance/eigen kernel (s1 == s2: plain in-order issue on one stream).
static int issue_group(const ExtractCall &c, int g0, int g1, hipStream_t s1, hipStream_t s2, hipEvent_t after_first,
                       hipEvent_t after_second, bool split)
{
    salsa_plan *pl = c.pl;
    KParams gp = c.kp;
    gp.B = g1 - g0;
    const long T = gp.T;
    const float *a = c.audio + (size_t)g0 * 4 * gp.N;
    float *o = c.out + (size_t)g0 * 7 * T * gp.F;
    float4 *xs = nullptr;
    unsigned *vm = nullptr;
    if (c.full) bind_workspace(c.lay, c.ws, g0, c.doubt, xs, vm, gp);
    const bool two = split && c.full && gp.nd > 0;
    gp.pair_sel = two ? 0 : -1;
    int rc = timed(pl, s1, "stft_logspec", REPEATABLE, [&] { return launch_k1(pl, gp, a, o, xs, s1); });
    if (rc || !c.full) return rc;
    if (pl->stop_after == 1) return SALSA_PARTIAL; // (measurement mode: the caller is told the outputs are NOT complete)
    if (s1 != s2) {
        HIP_TRY(hipEventRecord(after_first, s1));
        HIP_TRY(hipStreamWaitEvent(s2, after_first, 0));
    }
    if (gp.nd == 0) { // empty DOA band: channels 4-6 are all zero (:373-374)
        HIP_TRY(hipMemset2DAsync(o + 4 * T * gp.F, sizeof(float) * 7 * T * gp.F, 0, sizeof(float) * 3 * T * gp.F, (size_t)gp.B, s2));
        return SALSA_OK;
    }
    if (two) { // channels 2/3 (the tracker below only needs channel 0 and may run beside this launch)
        gp.pair_sel = 1;
        rc = timed(pl, s1, "stft_logspec", ONCE, [&] { return launch_stft(pl, gp, pl->d_window, a, o, xs, s1); });
        if (rc) return rc;
        gp.pair_sel = -1;
        if (s1 != s2) HIP_TRY(hipEventRecord(after_second, s1));
    }
    if (gp.tracking) {
        timed(pl, s2, "noise_floor_tracker", REPEATABLE, [&] { return launch_tracker(gp, s2, xs, vm), (int)SALSA_OK; });
        HIP_TRY(hipGetLastError());
    }
    if (pl->stop_after == 2) return SALSA_PARTIAL;
    if (two && s1 != s2) HIP_TRY(hipStreamWaitEvent(s2, after_second, 0));
    // stage (a): the fused kernel on the masks of the launches above; its float64 records go where the group's spill was (dead
    // once the tracker has read it: same stream)
    if (pl->fused >= 1 && !two && fused_eligible(pl, gp) && fused_cold_bytes(gp) <= c.lay.spill_group_bytes(gp.B))
        return timed(pl, s2, "fused_stft_cov_eig", REPEATABLE, [&] { return launch_fused(pl, gp, a, o, vm, (void *)xs, s2); });
    const unsigned ntile = (unsigned)((gp.T + K3_FT - 1) / K3_FT);
    dim3 grid(ntile, (unsigned)gp.B, (unsigned)((gp.nd + K3_NT - 1) / K3_NT));
    timed(pl, s2, "cov_eig", REPEATABLE,
          [&] { return launch_cov_eig<true>(gp, grid, s2, xs, vm, o, (double *)nullptr, (unsigned char *)nullptr), (int)SALSA_OK; });
    HIP_TRY(hipGetLastError());
    if (gp.flex && !gp.tracking && gp.nd > 0) { // (it consumes the marks cov_eig left: not repeatable)
        timed(pl, s2, "flex_allpass", ONCE, [&] { return launch_flex_allpass(gp, s2, o), (int)SALSA_OK; });
        HIP_TRY(hipGetLastError());
    }
    return SALSA_OK;
}

// the pipelined schedule: fork from `origin`, run the batch as G clip groups on the plan's streams, join back into `origin`
static int issue_forked(const ExtractCall &c, int G, hipStream_t origin)
{
    salsa_plan *pl = c.pl;
    const int batch = c.kp.B;
    const bool split = (pl->pipe_flags & SALSA_PIPE_SPLIT_PAIRS) != 0;
    HIP_TRY(hipEventRecord(pl->ev_fork, origin));
    HIP_TRY(hipStreamWaitEvent(pl->streams[0], pl->ev_fork, 0));
    for (int g = 0; g < G; g++) {
        HIP_TRY(hipStreamWaitEvent(pl->streams[1 + g], pl->ev_fork, 0)); // orders this call after the caller's earlier work
        const int g0 = (int)((long)batch * g / G), g1 = (int)((long)batch * (g + 1) / G);
        const int rc = issue_group(c, g0, g1, pl->streams[0], pl->streams[1 + g], pl->ev_stft[g], pl->ev_stft2[g], split);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(pl->ev_join[1 + g], pl->streams[1 + g]));
        HIP_TRY(hipStreamWaitEvent(origin, pl->ev_join[1 + g], 0));
    }
    HIP_TRY(hipEventRecord(pl->ev_join[0], pl->streams[0]));
    HIP_TRY(hipStreamWaitEvent(origin, pl->ev_join[0], 0));
    return SALSA_OK;
}

// one hipGraphLaunch per call: the fork/join above, captured once for these buffers and sizes (the plan's graph key)
static int replay_graph(const ExtractCall &c, int G, hipStream_t s)
{
    salsa_plan *pl = c.pl;
    const salsa_plan::GraphKey key = {c.audio, c.out, c.ws, pl->sc_mean, pl->sc_std, c.kp.B, G, pl->pipe_flags, (int64_t)c.kp.N};
    if (!(pl->gexec && pl->gkey == key)) {
        if (pl->gexec) {
            (void)hipGraphExecDestroy(pl->gexec);
            pl->gexec = nullptr;
        }
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(pl->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = issue_forked(c, G, pl->cap_stream);
        const hipError_t e = hipStreamEndCapture(pl->cap_stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        HIP_TRY(e);
        const hipError_t ei = hipGraphInstantiate(&pl->gexec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HIP_TRY(ei);
        pl->gkey = key;
    }
    HIP_TRY(hipGraphLaunch(pl->gexec, s));
    return SALSA_OK;
}

// what the two salsa_eigvec entry points share once each has made its own checks: caller-supplied spectra relaid into the spill, the
// tracker, then the covariance / eigen kernel writing features (FEAT) or eigenvectors and gates
template <bool FEAT>
static int eigvec_run(salsa_plan *pl, const float *d_X, int batch, int n_bins, int64_t n_frames, int lower_bin, float *d_feat,
                      double *d_eig, unsigned char *d_gate, void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
    const WorkspaceLayout lay = workspace_layout(batch, (size_t)n_frames, n_bins, 4, MASK_CHUNKED);
    if (const int rc = refuse_workspace(d_workspace, workspace_bytes, lay.total)) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    KParams kp = make_kparams(pl, batch, 0);
    kp.T = (int)n_frames;
    kp.nd = n_bins;
    kp.lower = lower_bin;
    kp.upper = lower_bin + n_bins;
    kp.F = n_bins;
    kp.feature = SALSA_FEATURE_SALSA;
    float4 *Xs;
    unsigned *valid;
    bind_workspace(lay, d_workspace, 0, (kp.tracking || kp.flex) && kp.cond > 1.0, Xs, valid, kp);
    launch_relayout((const float4 *)d_X, Xs, batch, n_bins, (int)n_frames, s);
    HIP_TRY(hipGetLastError());
    if (kp.tracking) {
        launch_tracker(kp, s, Xs, valid);
        HIP_TRY(hipGetLastError());
    }
    const unsigned ntile = (unsigned)((kp.T + K3_FT - 1) / K3_FT);
    dim3 grid(ntile, (unsigned)kp.B, (unsigned)((n_bins + K3_NT - 1) / K3_NT));
    launch_cov_eig<FEAT>(kp, grid, s, Xs, valid, d_feat, d_eig, d_gate);
    HIP_TRY(hipGetLastError());
    return SALSA_OK;
}

} // namespace

extern "C" {

int salsa_abi_version(void) { return SALSA_ABI_VERSION; }
const char *salsa_build_flags(void) { return SALSA_BUILD_FLAGS; }
const char *salsa_last_error(void) { return g_err; }
// every translation unit's failures land in this one per-thread message (fail / HIP_TRY of salsa_internal.h; baseline_kernels.hip,
// bank_batch.hip); not part of the public ABI
SALSA_LOCAL void salsa_set_last_error_(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

int salsa_bin_limits(int fs, int n_fft, int fmin_doa, int fmax_doa, int *lower_bin, int *upper_bin, int *cutoff_bin)
{
    if (fs <= 0 || n_fft <= 0 || !lower_bin || !upper_bin) return fail(SALSA_EINVAL, "salsa_bin_limits: bad argument%s");
    // salsa_feature_extraction.py:298-304: fmax = min(fmax, fs//2); int(floor(f * n_fft / float(fs))); lower = max(1, lower)
    const int fmax = fmax_doa < fs / 2 ? fmax_doa : fs / 2;
    int lo = (int)floor((double)((int64_t)fmin_doa * n_fft) / (double)fs);
    const int up = (int)floor((double)((int64_t)fmax * n_fft) / (double)fs);
    if (lo < 1) lo = 1;
    *lower_bin = lo;
    *upper_bin = up;
    if (cutoff_bin) *cutoff_bin = (int)floor((double)((int64_t)9000 * n_fft) / (double)fs); // lite :57-58
    return SALSA_OK;
}

static int freq_dim(int n_fft, int compress)
{
    if (n_fft != 512 && n_fft != 256) return -1;
    if (compress) return n_fft == 512 ? 200 : 100;
    return n_fft / 2;
}

int salsa_compress_matrix(int n_fft, int compress, float *W)
{
    const int F = freq_dim(n_fft, compress);
    if (F < 0) return fail(SALSA_ENFFT, "nfft is not 512 or 256%s");
    if (!W) return fail(SALSA_EINVAL, "salsa_compress_matrix: NULL output%s");
    const int nb = n_fft / 2 + 1;
    memset(W, 0, sizeof(float) * (size_t)F * nb);
    const int ident = compress ? (n_fft == 512 ? 192 : 96) : n_fft / 2;
    for (int i = 0; i < ident; i++) W[(size_t)i * nb + i + 1] = 1.0f;
    for (int i = ident; i < F; i++) {
        const int cnt = i < F - 1 ? 8 : 7;
        for (int k = 0; k < cnt; k++) W[(size_t)i * nb + ident + 1 + (i - ident) * 8 + k] = 0.125f;
    }
    return SALSA_OK;
}

// the plan's bands from its parameters: the DOA band [lower, upper) of nd bins, the spectrogram band, the F feature bins per frame
static int plan_bands(salsa_plan *pl)
{
    const salsa_params &p = pl->p;
    salsa_bin_limits(p.fs, p.n_fft, p.fmin_doa, p.fmax_doa, &pl->lower, &pl->upper, &pl->cutoff);
    const int nbins = p.n_fft / 2 + 1;
    if (pl->flex) {
        // contrib/salsa_flexible.py SpatialFeaturesAbstract.__init__ (:177-184) + __call__ (:252-263): no fs/2 clamp on
        // fmax_doa, the spectrogram cutoff comes from fmax_spec, spectrogram and spatial features share ONE band
        // [lo, hi) (the cropped axis, or all n_fft/2+1 bins), spatial rows >= upper_bin OF THAT AXIS optionally zeroed.
        if (p.audio_format != SALSA_FORMAT_MIC || p.feature_type == SALSA_FEATURE_IPD)
            return fail(SALSA_EFORMAT, "the contrib (flex) surface has the MIC-style SALSA and SALSA-Lite features only%s");
        pl->upper = (int)floor((double)((int64_t)p.fmax_doa * p.n_fft) / (double)p.fs);
        pl->cutoff = (int)floor((double)((int64_t)(p.fmax_spec > 0 ? p.fmax_spec : 9000) * p.n_fft) / (double)p.fs);
        if (pl->upper > pl->cutoff)
            return fail(SALSA_EBINS, "Upper bin for spatial feature is higher than cutoff bin for spectrogram!%s");
        const bool crop = !(p.flags & SALSA_FLAG_NO_CLIP_FREQS);
        const int lo = crop ? pl->lower : 0, hi = crop ? (pl->cutoff < nbins ? pl->cutoff : nbins) : nbins;
        const int zero_from = (p.flags & SALSA_FLAG_CLIP_SPATIAL_ALIAS) ? pl->upper : hi - lo; // index into the band
        pl->lower = lo;
        pl->cutoff = hi;
        pl->F = hi - lo;
        if (pl->F <= 0) return fail(SALSA_EBINS, "empty spectrogram band%s");
        pl->ident = p.n_fft / 2;
        pl->spec_lo = lo;
        pl->spec_hi = hi;
        if (p.feature_type == SALSA_FEATURE_SALSA) {
            pl->nd = zero_from < pl->F ? zero_from : pl->F; // bins above it are never evaluated: cov_eig zero-fills them
            pl->upper = lo + pl->nd;
        } else {
            pl->nd = 0;
            pl->upper = zero_from;                           // the lite kernel zeroes band rows >= kp.upper
        }
    } else if (p.feature_type == SALSA_FEATURE_SALSA) {
        pl->F = freq_dim(p.n_fft, p.is_compress_high_freq);
        pl->ident = p.is_compress_high_freq ? (p.n_fft == 512 ? 192 : 96) : p.n_fft / 2;
        pl->spec_lo = 1;
        pl->spec_hi = pl->ident + 1;
        pl->nd = pl->upper - pl->lower;
        if (pl->nd < 0 || pl->nd > pl->F || pl->upper > nbins)
            return fail(SALSA_EBINS, "DOA band [lower_bin, upper_bin) does not fit the feature axis%s");
    } else {
        if (pl->upper > pl->cutoff)
            return fail(SALSA_EBINS, "Upper bin for spatial feature is higher than cutoff bin for spectrogram!%s");
        if (pl->cutoff > nbins) pl->cutoff = nbins; // numpy slicing clips [lower:cutoff] at n_bins
        pl->F = pl->cutoff - pl->lower;
        pl->ident = 0;
        pl->nd = 0;
        if (pl->F <= 0) return fail(SALSA_EBINS, "empty spectrogram band%s");
    }
    return SALSA_OK;
}

// windows: scipy.signal.get_window('hann', win, fftbins=True), centre-padded to n_fft (librosa pad_center: (n_fft - win) // 2
// zeros on the left) ; twiddles W_N^m.  Only the SALSA log-spectrogram honours win_len (salsa_feature_extraction.py:186-192); its
// DOA STFT (:360-361) and both SALSA-Lite STFTs (salsa_lite_feature_extraction.py:97-98, win_len read at :44 and unused) pass no
// win_length, i.e. the n_fft window.  Equal lengths: one table.
static int plan_upload_tables(salsa_plan *pl)
{
    const int n_fft = pl->p.n_fft;
    const int spec_win = (pl->p.feature_type == SALSA_FEATURE_SALSA && !pl->flex) ? pl->p.win_len : n_fft;
    const int nwin = spec_win == n_fft ? 1 : 2;
    std::vector<double> hw(2 * n_fft, 0.0);
    std::vector<cplx<double>> htw(n_fft);
    for (int n = 0; n < spec_win; n++) hw[(n_fft - spec_win) / 2 + n] = 0.5 - 0.5 * cos(2.0 * PI * n / spec_win);
    for (int n = 0; n < n_fft; n++) hw[n_fft + n] = 0.5 - 0.5 * cos(2.0 * PI * n / n_fft);
    for (int m = 0; m < n_fft; m++) htw[m] = {cos(-2.0 * PI * m / n_fft), sin(-2.0 * PI * m / n_fft)};
    hipError_t e1 = hipMalloc((void **)&pl->d_window, sizeof(double) * n_fft * nwin);
    hipError_t e2 = hipMalloc((void **)&pl->d_tw, sizeof(cplx<double>) * n_fft);
    if (e1 == hipSuccess && e2 == hipSuccess) {
        e1 = hipMemcpy(pl->d_window, hw.data(), sizeof(double) * n_fft * nwin, hipMemcpyHostToDevice);
        e2 = hipMemcpy(pl->d_tw, htw.data(), sizeof(cplx<double>) * n_fft, hipMemcpyHostToDevice);
    }
    if (e1 != hipSuccess || e2 != hipSuccess)
        return fail(SALSA_EHIP, "plan table upload failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    pl->d_window_doa = nwin == 2 ? pl->d_window + n_fft : pl->d_window;
    return SALSA_OK;
}

int salsa_plan_create(const salsa_params *params, salsa_plan **out_plan)
{
    if (!params || !out_plan) return fail(SALSA_EINVAL, "salsa_plan_create: NULL argument%s");
    const salsa_params &p = *params;
    // full SALSA: the reference's own assert (salsa_feature_extraction.py:152, :306).  Its SALSA-Lite / IPD script has none; here those
    // two features also take 1024 (stft_kernel<1024, ...>), on the dataset scripts' surface (not contrib's SALSA_FLAG_FLEX); every other size is refused
    const bool lite_1024 = p.n_fft == 1024 && (p.feature_type == SALSA_FEATURE_LITE || p.feature_type == SALSA_FEATURE_IPD) && !(p.flags & SALSA_FLAG_FLEX);
    if (p.n_fft != 512 && p.n_fft != 256 && !lite_1024) {
        if (p.feature_type == SALSA_FEATURE_LITE || p.feature_type == SALSA_FEATURE_IPD)
            return fail(SALSA_ENFFT, "only 256, 512 or 1024 fft is supported for SALSA-Lite and SALSA-IPD (256 or 512 with the contrib flags)%s");
        return fail(SALSA_ENFFT, "only 256 or 512 fft is supported%s");
    }
    if (p.fs <= 0 || p.hop_len <= 0 || p.win_len <= 0 || p.win_len > p.n_fft)
        return fail(SALSA_EINVAL, "bad fs / hop_len / win_len (window length must be <= nfft)%s");
    if (p.audio_format != SALSA_FORMAT_FOA && p.audio_format != SALSA_FORMAT_MIC)
        return fail(SALSA_EFORMAT, "Unknown audio format%s");
    if (p.feature_type < SALSA_FEATURE_SALSA || p.feature_type > SALSA_FEATURE_IPD)
        return fail(SALSA_EINVAL, "Invalid feature type%s");
    if (p.feature_type != SALSA_FEATURE_SALSA && p.audio_format != SALSA_FORMAT_MIC)
        return fail(SALSA_EFORMAT, "SALSA-Lite and SALSA-IPD are only for MIC format!%s");
    if (p.n_hopframes < 0 || p.n_hopframes > 16) return fail(SALSA_EINVAL, "n_hopframes out of range%s");
    // the plan, and whatever device memory it comes to hold, is released by every refusal below: one `return` each
    std::unique_ptr<salsa_plan, int (*)(salsa_plan *)> pl(new salsa_plan(), salsa_plan_destroy);
    memset(pl.get(), 0, sizeof(salsa_plan));
    pl->p = p;
    pl->flex = (p.flags & SALSA_FLAG_FLEX) != 0;
    pl->snr_ratio = p.floor_mask_ratio > 0 ? p.floor_mask_ratio : 1.5;
    if (const int rc = plan_bands(pl.get())) return rc;
    pl->delta = 2.0 * PI * p.fs / (p.n_fft * 343.0);
    if (hipGetDevice(&pl->device) != hipSuccess) return fail(SALSA_EHIP, "hipGetDevice failed (no HIP device?)%s");
    if (const int rc = plan_upload_tables(pl.get())) return rc;
    pl->n_groups = 1; // measured on ROCm 7.2: multi-stream issue costs more host time than the overlap returns
    *out_plan = pl.release();
    return SALSA_OK;
}

int salsa_plan_destroy(salsa_plan *pl)
{
    if (!pl) return SALSA_OK;
    if (pl->d_window) (void)hipFree(pl->d_window);
    if (pl->d_tw) (void)hipFree(pl->d_tw);
    for (int i = 0; i < SALSA_MAX_KERNELS; i++) {
        if (pl->ev0[i]) (void)hipEventDestroy(pl->ev0[i]);
        if (pl->ev1[i]) (void)hipEventDestroy(pl->ev1[i]);
    }
    for (int i = 0; i <= SALSA_MAX_GROUPS; i++) {
        if (pl->streams[i]) (void)hipStreamDestroy(pl->streams[i]);
        if (pl->ev_join[i]) (void)hipEventDestroy(pl->ev_join[i]);
        if (i < SALSA_MAX_GROUPS && pl->ev_stft[i]) (void)hipEventDestroy(pl->ev_stft[i]);
        if (i < SALSA_MAX_GROUPS && pl->ev_stft2[i]) (void)hipEventDestroy(pl->ev_stft2[i]);
    }
    if (pl->gexec) (void)hipGraphExecDestroy(pl->gexec);
    if (pl->cap_stream) (void)hipStreamDestroy(pl->cap_stream);
    if (pl->ev_fork) (void)hipEventDestroy(pl->ev_fork);
    delete pl;
    return SALSA_OK;
}

int salsa_output_shape(const salsa_plan *pl, int64_t n_samples, int *C, int64_t *T, int *F)
{
    if (!pl || n_samples < 0) return fail(SALSA_EINVAL, "salsa_output_shape: bad argument%s");
    if (C) *C = 7;
    if (T) *T = 1 + n_samples / pl->p.hop_len;
    if (F) *F = pl->F;
    return SALSA_OK;
}

// (what the workspace holds and how large it is: salsa_workspace.h)
size_t salsa_workspace_bytes(const salsa_plan *pl, int batch, int64_t n_samples)
{
    if (!pl || batch <= 0 || n_samples <= 0 || pl->p.feature_type != SALSA_FEATURE_SALSA) return 0;
    return workspace_layout(batch, (size_t)(1 + n_samples / pl->p.hop_len), pl->nd, 4, MASK_CHUNKED).total;
}

size_t salsa_eigvec_workspace_bytes(const salsa_plan *pl, int batch, int n_bins, int64_t n_frames)
{
    if (!pl || batch <= 0 || n_bins <= 0 || n_frames <= 0) return 0;
    return workspace_layout(batch, (size_t)n_frames, n_bins, 4, MASK_CHUNKED).total;
}

int salsa_extract_batch(salsa_plan *pl, const float *d_audio, int batch, int64_t n_samples, float *d_out,
                        void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!pl || !d_audio || !d_out || batch <= 0 || n_samples <= 0)
        return fail(SALSA_EINVAL, "salsa_extract_batch: bad argument%s");
    if (const int rc = refuse_short_clip(pl, n_samples)) return rc;
    if (const int rc = refuse_other_device(pl)) return rc;
    {   // kernels index inside one clip with 32-bit offsets
        const int64_t T64 = 1 + n_samples / pl->p.hop_len;
        if (n_samples * 16 >= INT32_MAX || T64 * 7 * pl->F >= INT32_MAX / 2 || T64 * 2 * (pl->nd > 0 ? pl->nd : 1) >= INT32_MAX / 8)
            return fail(SALSA_EINVAL, "clip too long for 32-bit per-clip indexing (split it)%s");
        if ((T64 + K3_FT - 1) / K3_FT > 65535) return fail(SALSA_EINVAL, "clip too long for one launch (split it)%s");
    }
    hipStream_t s = (hipStream_t)hip_stream;
    ExtractCall c = {pl, make_kparams(pl, batch, n_samples), d_audio, d_out, pl->p.feature_type == SALSA_FEATURE_SALSA, d_workspace};
    if (c.full) {
        c.lay = workspace_layout(batch, (size_t)c.kp.T, c.kp.nd, 4, MASK_CHUNKED);
        if (const int rc = refuse_workspace(d_workspace, workspace_bytes, c.lay.total)) return rc;
        c.doubt = (c.kp.tracking || c.kp.flex) && c.kp.cond > 1.0 && c.kp.nd > 0;
    }
    pl->n_kernels = 0;
    // (a plan with two windows keeps the plain in-order schedule: the pipelined one launches K1 per channel pair with one window)
    const bool piped = c.full && !pl->timing && !pl->stop_after && c.kp.nd > 0 && pl->d_window == pl->d_window_doa &&
                       (pl->n_groups > 1 || (pl->pipe_flags & SALSA_PIPE_SPLIT_PAIRS));
    if (!piped) return issue_group(c, 0, batch, s, s, nullptr, nullptr, false);
    const int G = batch < pl->n_groups ? batch : pl->n_groups;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (s) (void)hipStreamIsCapturing(s, &cap);
    if (!(pl->pipe_flags & SALSA_PIPE_GRAPH) || cap != hipStreamCaptureStatusNone)
        return issue_forked(c, G, s); // eager fork/join (inside a caller's capture it becomes part of the caller's graph)
    return replay_graph(c, G, s);
}

int salsa_logspec_batch(salsa_plan *pl, const float *d_audio, int batch, int n_channels, int64_t n_samples,
                        float *d_out, void *hip_stream)
{
    if (!pl || !d_audio || !d_out || batch <= 0 || n_samples <= 0) return fail(SALSA_EINVAL, "salsa_logspec_batch: bad argument%s");
    if (n_channels != 4) return fail(SALSA_EINVAL, "salsa_logspec_batch: n_channels must be 4 (pad with silent channels)%s");
    if (freq_dim(pl->p.n_fft, pl->p.is_compress_high_freq) < 0) return fail(SALSA_ENFFT, "nfft is not 512 or 256%s"); // (MagStftExtractor, :152)
    if (const int rc = refuse_short_clip(pl, n_samples)) return rc;
    if (n_samples * 16 >= INT32_MAX || (1 + n_samples / pl->p.hop_len) * 7 * 256 >= INT32_MAX / 2)
        return fail(SALSA_EINVAL, "clip too long for 32-bit per-clip indexing (split it)%s");
    KParams kp = make_kparams(pl, batch, n_samples);
    kp.feature = FEATURE_LOGSPEC_ONLY;
    kp.OC = 4;
    kp.sc_mean = kp.sc_std = nullptr; // MagStftExtractor.extract returns raw dB
    kp.layout = SALSA_LAYOUT_PLANAR;
    kp.F = freq_dim(pl->p.n_fft, pl->p.is_compress_high_freq);
    kp.ident = pl->p.is_compress_high_freq ? (pl->p.n_fft == 512 ? 192 : 96) : pl->p.n_fft / 2;
    kp.compress = pl->p.is_compress_high_freq;
    kp.spec_lo = 1;
    kp.spec_hi = kp.ident + 1;
    return launch_stft(pl, kp, pl->d_window, d_audio, d_out, nullptr, (hipStream_t)hip_stream); // (the spectrogram window: win_len)
}

int salsa_eigvec_batch(salsa_plan *pl, const float *d_X, int batch, int n_bins, int64_t n_frames, int lower_bin,
                       double *d_out, unsigned char *d_gate, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream)
{
    if (!pl || !d_X || !d_out || batch <= 0 || n_bins <= 0 || n_frames <= 0)
        return fail(SALSA_EINVAL, "salsa_eigvec_batch: bad argument%s");
    if ((int64_t)n_frames * 2 * n_bins >= INT32_MAX) return fail(SALSA_EINVAL, "block too large for 32-bit per-clip indexing%s");
    return eigvec_run<false>(pl, d_X, batch, n_bins, n_frames, lower_bin, nullptr, d_out, d_gate, d_workspace, workspace_bytes, hip_stream);
}

int salsa_eigvec_feature_batch(salsa_plan *pl, const float *d_X, int batch, int n_bins, int64_t n_frames, int lower_bin,
                               float *d_feat, void *d_workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!pl || !d_X || !d_feat || batch <= 0 || n_bins <= 0 || n_frames <= 0)
        return fail(SALSA_EINVAL, "salsa_eigvec_feature_batch: bad argument%s");
    if ((int64_t)n_frames * 2 * n_bins >= INT32_MAX / 8 || (int64_t)n_frames * 7 * n_bins >= INT32_MAX / 2)
        return fail(SALSA_EINVAL, "block too large for 32-bit per-clip indexing%s");
    if ((n_frames + K3_FT - 1) / K3_FT > 65535) return fail(SALSA_EINVAL, "block too long for one launch%s");
    return eigvec_run<true>(pl, d_X, batch, n_bins, n_frames, lower_bin, d_feat, nullptr, nullptr, d_workspace, workspace_bytes, hip_stream);
}

int salsa_plan_set_fused(salsa_plan *pl, int mode)
{
    if (!pl || mode < 0 || mode > 2) return fail(SALSA_EINVAL, "salsa_plan_set_fused: bad argument%s");
    pl->fused = mode;
    return SALSA_OK;
}

int salsa_plan_set_stats(salsa_plan *pl, unsigned long long *d_counters)
{
    if (!pl) return fail(SALSA_EINVAL, "salsa_plan_set_stats: NULL plan%s");
    pl->stats = d_counters;
    return SALSA_OK;
}

int salsa_plan_set_timing(salsa_plan *pl, int enable)
{
    if (!pl) return fail(SALSA_EINVAL, "salsa_plan_set_timing: NULL plan%s");
    pl->timing = enable > 0 ? enable : 0; // 1: an event pair around every launch; K > 1: K launches per event pair
    pl->stop_after = enable < 0 ? (enable >= -2 ? -enable : 0) : 0; // -1 / -2: plain issue of a PREFIX of the path (no events)
    pl->n_kernels = 0;
    return SALSA_OK;
}

int salsa_plan_read_timing(salsa_plan *pl, float *ms, const char **names, int *n_out)
{
    if (!pl || !ms || !n_out) return fail(SALSA_EINVAL, "salsa_plan_read_timing: NULL argument%s");
    *n_out = 0;
    if (!pl->timing || pl->n_kernels == 0) return SALSA_OK;
    for (int i = 0; i < pl->n_kernels; i++) {
        HIP_TRY(hipEventSynchronize(pl->ev1[i]));
        HIP_TRY(hipEventElapsedTime(&ms[i], pl->ev0[i], pl->ev1[i]));
        if (pl->timing > 1) ms[i] /= (float)pl->timing; // per launch
        if (names) names[i] = pl->names[i];
    }
    *n_out = pl->n_kernels;
    return SALSA_OK;
}

static int ensure_group_streams(salsa_plan *pl)
{
    if (pl->streams[0]) return SALSA_OK;
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi); // hi = numerically lowest = highest priority
    bool ok = true;
    for (int i = 0; i <= SALSA_MAX_GROUPS && ok; i++)
        ok = hipStreamCreateWithPriority(&pl->streams[i], hipStreamNonBlocking, i == 0 ? lo : hi) == hipSuccess;
    ok = ok && hipStreamCreateWithFlags(&pl->cap_stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < SALSA_MAX_GROUPS && ok; i++)
        ok = hipEventCreateWithFlags(&pl->ev_stft[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&pl->ev_stft2[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i <= SALSA_MAX_GROUPS && ok; i++) ok = hipEventCreateWithFlags(&pl->ev_join[i], hipEventDisableTiming) == hipSuccess;
    return ok ? SALSA_OK : fail(SALSA_EHIP, "stream / event creation failed%s");
}

int salsa_plan_set_scaler(salsa_plan *pl, const float *d_mean, const float *d_std)
{
    if (!pl || ((d_mean == nullptr) != (d_std == nullptr))) return fail(SALSA_EINVAL, "salsa_plan_set_scaler: bad argument%s");
    pl->sc_mean = d_mean;
    pl->sc_std = d_std;
    return SALSA_OK;
}

int salsa_plan_set_pipeline(salsa_plan *pl, int n_groups, int flags)
{
    if (!pl || n_groups < 1 || (flags & ~(SALSA_PIPE_SPLIT_PAIRS | SALSA_PIPE_GRAPH)))
        return fail(SALSA_EINVAL, "salsa_plan_set_pipeline: bad argument%s");
    if (n_groups > 1 || (flags & SALSA_PIPE_SPLIT_PAIRS)) { // the plan-owned streams are only created when a pipeline is requested
        const int rc = ensure_group_streams(pl);
        if (rc) return rc;
    }
    pl->n_groups = n_groups > SALSA_MAX_GROUPS ? SALSA_MAX_GROUPS : n_groups;
    pl->pipe_flags = flags;
    return SALSA_OK;
}

int salsa_plan_set_groups(salsa_plan *pl, int n_groups)
{
    if (!pl) return fail(SALSA_EINVAL, "salsa_plan_set_groups: bad argument%s");
    return salsa_plan_set_pipeline(pl, n_groups, pl->pipe_flags);
}

} // extern "C"
