/*
 * salsa_hip.h -- C ABI of libsalsa_hip.so, the MI355X (gfx950) SALSA / SALSA-Lite feature extractor.
 *
 * The upstream reference (thomeou/SALSA) is pure Python and has no FFI layer: its boundary is a set of Python
 * function signatures plus the (7, T, F) float32 feature array they produce.  Each entry point below replaces one of
 * those, batched over clips and operating on caller-owned DEVICE memory (plain pointers and sizes, no torch types);
 * salsa_amd/features.py re-exposes the reference's own signatures on top of them.
 *
 *   reference interface (file:line, relative to the upstream repo)               replaced by
 *   ---------------------------------------------------------------------------  ---------------------------------
 *   extract_features() per-file body, dataset/salsa_feature_extraction.py:353-377 salsa_extract_batch (SALSA)
 *   extract_features() per-file body, dataset/salsa_lite_feature_extraction.py:94-123  salsa_extract_batch (LITE/IPD)
 *   MagStftExtractor.extract, dataset/salsa_feature_extraction.py:177-201         salsa_logspec_batch
 *   extract_normalized_eigenvector, dataset/salsa_feature_extraction.py:17-129    salsa_eigvec_batch
 *   bin limits / freq_dim, dataset/salsa_feature_extraction.py:298-313 (+ lite :50-59)  salsa_bin_limits, salsa_output_shape
 *   MagStftExtractor.W, dataset/salsa_feature_extraction.py:152-175               salsa_compress_matrix (host)
 *   compute_scaler, dataset/salsa_feature_extraction.py:204-262                   salsa_scaler_accumulate
 *   Database.load_chunk_data normalisation, dataset/database.py:197-202           salsa_normalize_batch
 *   SeldDataset train transforms, utilities/transforms.py (datamodule.py:45-82)   salsa_augment_batch
 *   SalsaFeatures / SalsaLiteFeatures.__call__, contrib/salsa_flexible.py:237-265 (+ :286-400)   salsa_extract_batch with SALSA_FLAG_FLEX, salsa_to_freq_major
 *   librosa.load(sr=fs)'s resampling of a file of another rate, dataset/salsa_feature_extraction.py:353   salsa_resample_batch
 *   librosa.load's PCM -> float32 (channels, samples) conversion, dataset/salsa_feature_extraction.py:353    salsa_pcm_to_planar
 *
 * Conventions: every function returns 0 on success or a negative SALSA_E* code; salsa_last_error() gives the
 * message of the calling thread's last failure.  Device pointers are caller-owned; work is enqueued asynchronously
 * on the HIP stream passed in (NULL = the default stream) and nothing is allocated or synchronised inside the
 * extract calls, so they are hipGraph-capturable.  A plan is bound to the device current at salsa_plan_create.
 */
#ifndef SALSA_HIP_H
#define SALSA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALSA_ABI_VERSION 2

enum { SALSA_FORMAT_FOA = 0, SALSA_FORMAT_MIC = 1 };                      /* cfg['data']['format'] */
enum { SALSA_FEATURE_SALSA = 0, SALSA_FEATURE_LITE = 1, SALSA_FEATURE_IPD = 2 }; /* 'salsa' | 'salsa_lite' | 'salsa_ipd' */
enum { SALSA_LAYOUT_PLANAR = 0, SALSA_LAYOUT_INTERLEAVED = 1 };           /* [B][4][N] (librosa.load) | [B][N][4] (WAV) */

/* salsa_params.flags.  SALSA_FLAG_FLEX selects the semantics of the on-the-fly re-implementation contrib/salsa_flexible.py
 * (MIC-style features only), which differ from the dataset scripts: the noise-floor tracker follows the raw |X0| (not the
 * 3-frame RMS) with its initial floor clamped to 1e-6 (:118-120, :326-333); the coherence test gates even without
 * tracking -- and then switches a bin off for the rest of the clip once it fails (:336-337, :352-354); the frequency
 * normalisation vector is float32 (:188-190); the log-spectrogram is uncompressed over the SAME band as the spatial
 * features: bins [lower_bin, cutoff_bin(fmax_spec)) or, with SALSA_FLAG_NO_CLIP_FREQS, all n_fft/2+1 bins
 * (clip_freqs, :252-257); SALSA_FLAG_CLIP_SPATIAL_ALIAS zeroes spatial rows >= upper_bin of that band
 * (clip_spatial_alias, :262-263); fmax_doa is not clamped to fs/2.  cond_num = ew_thresh, n_hopframes =
 * covmat_avg_neighbours.  Fewer than 4 microphones: pad the audio with silent channels (the covariance gains zero
 * eigenvalues, the gate and the principal eigenvector are unchanged) and drop the padded output channels. */
enum { SALSA_FLAG_FLEX = 1, SALSA_FLAG_NO_CLIP_FREQS = 2, SALSA_FLAG_CLIP_SPATIAL_ALIAS = 4,
       /* verification switch: salsa_extract_batch / salsa_eigvec_feature_batch launch the all-float64 instantiation of the
        * covariance + eigen kernel instead of the production packed-float32 pair solve with its float64 cold list (same
        * spill, same masks), so a test can hold the two against each other on the GPU. */
       SALSA_FLAG_FORCE_F64 = 8 };

enum {
    SALSA_OK = 0,
    SALSA_PARTIAL = 1,     /* measurement mode only (salsa_plan_set_timing(plan, -1 | -2)): a PREFIX of the path was issued, the
                            * output planes hold whatever an earlier full call left there -- never returned by a plain call */
    SALSA_EINVAL = -1,     /* bad argument (NULL pointer, negative size, ...) */
    SALSA_ENFFT = -2,      /* full SALSA: n_fft not in {256, 512}, the reference's assert, salsa_feature_extraction.py:152,306.
                            * SALSA-Lite / SALSA-IPD (whose script has no such assert): n_fft not in {256, 512, 1024} -- a restriction of
                            * this library; 1024 is not taken with SALSA_FLAG_FLEX, nor by salsa_logspec_batch / salsa_compress_matrix */
    SALSA_EFORMAT = -3,    /* unknown audio format: the reference's ValueError, :125,:332 ; lite requires MIC, lite :72 */
    SALSA_EBINS = -4,      /* upper_bin > cutoff_bin (lite :59) or an empty / oversized DOA band */
    SALSA_EWORKSPACE = -5, /* workspace smaller than salsa_workspace_bytes() */
    SALSA_EHIP = -6        /* a HIP runtime call failed (message in salsa_last_error) */
};

/* Mirrors the keyword arguments of the reference's extract_features() + the cfg['data'] block of its YAML. */
typedef struct salsa_params {
    int fs;                    /* 24000 */
    int n_fft;                 /* 512 | 256 */
    int hop_len;               /* 300 */
    int win_len;               /* <= n_fft: the Hann window of the SALSA log-spectrogram channels only (centre-padded to n_fft, as
                                * librosa's pad_center).  The DOA spectra of SALSA and every SALSA-Lite / IPD channel use the n_fft
                                * Hann window, as in the reference (salsa_feature_extraction.py:186-192 vs :360-361; the Lite script
                                * reads win_len and never uses it).  A SALSA plan with win_len < n_fft runs the STFT kernel twice
                                * (DOA window, then spectrogram window) and always the three-kernel schedule: the fused kernel and
                                * the pipelined schedules fall back to it, with the same results. */
    int fmin_doa;              /* Hz */
    int fmax_doa;              /* Hz (clamped to fs/2 like the reference) */
    double cond_num;           /* coherence threshold, default 5 */
    int n_hopframes;           /* default 3 ("do not change") */
    int is_tracking;           /* noise-floor tracking */
    int is_compress_high_freq; /* 200/100-bin compressed log-spectrogram */
    int audio_format;          /* SALSA_FORMAT_* */
    int feature_type;          /* SALSA_FEATURE_* */
    int audio_layout;          /* SALSA_LAYOUT_* */
    int flags;                 /* SALSA_FLAG_* (0 = the dataset scripts' semantics) */
    double floor_mask_ratio;   /* indicator_sig = mag > ratio * floor; 0 = the reference's 1.5 (:36; contrib kwarg) */
    int fmax_spec;             /* SALSA_FLAG_FLEX only: spectrogram cutoff in Hz; 0 = 9000 */
    int reserved;
} salsa_params;

typedef struct salsa_plan salsa_plan;

int salsa_abi_version(void);
/* "" for the product's build (salsa_amd/_lib.py build_command(): no -D at all).  Otherwise what this library was built with: " PROBE"
 * when -DSALSA_PROBE_BUILD admitted the timing-probe switches of salsa_amd/csrc (most of which compute wrong results on purpose), then
 * " NAME=value" for every overridden tunable -- so that an A/B or probe library loaded in place of the product identifies itself. */
const char *salsa_build_flags(void);
const char *salsa_last_error(void);

/* lower_bin, upper_bin (exclusive) and the lite spectrogram cutoff bin, bit-exact integer arithmetic of the reference */
int salsa_bin_limits(int fs, int n_fft, int fmin_doa, int fmax_doa, int *lower_bin, int *upper_bin, int *cutoff_bin);
/* host: the (freq_dim x n_fft/2+1) float32 row-major compression matrix W (what the kernels apply implicitly) */
int salsa_compress_matrix(int n_fft, int is_compress_high_freq, float *W_host);

int salsa_plan_create(const salsa_params *params, salsa_plan **out_plan);
int salsa_plan_destroy(salsa_plan *plan);
/* feature array shape for clips of n_samples: C = 7, T = 1 + n_samples / hop_len, F = 200 | 100 | n_fft/2 | cutoff-lower */
int salsa_output_shape(const salsa_plan *plan, int64_t n_samples, int *C, int64_t *T, int *F);
/* scratch bytes salsa_extract_batch needs for (batch, n_samples) */
size_t salsa_workspace_bytes(const salsa_plan *plan, int batch, int64_t n_samples);

/* d_audio: float32 [B][4][N] (planar) or [B][N][4] (interleaved) ; d_out: float32 [B][7][T][F], fully written. */
int salsa_extract_batch(salsa_plan *plan, const float *d_audio, int batch, int64_t n_samples, float *d_out,
                        void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* MagStftExtractor.extract: d_audio float32 [B][C][N] planar (any C that is a multiple of 2) -> d_out [B][C][T][F] */
int salsa_logspec_batch(salsa_plan *plan, const float *d_audio, int batch, int n_channels, int64_t n_samples,
                        float *d_out, void *hip_stream);

/* extract_normalized_eigenvector: d_X complex64 [B][n_bins][n_frames][4] (the reference's (n_bins,n_frames,n_chans)),
 * d_out float64 [B][3][n_bins][n_frames].  Uses plan's cond_num / n_hopframes / is_tracking / audio_format / fs /
 * n_fft; lower_bin as given (it only enters the MIC normalisation).  d_gate (optional, may be NULL): uint8
 * [B][n_bins][n_frames], 0 = rejected by the noise gate, 1 = failed the coherence test, 2 = emitted. */
size_t salsa_eigvec_workspace_bytes(const salsa_plan *plan, int batch, int n_bins, int64_t n_frames);
int salsa_eigvec_batch(salsa_plan *plan, const float *d_X, int batch, int n_bins, int64_t n_frames, int lower_bin,
                       double *d_out, unsigned char *d_gate, void *d_workspace, size_t workspace_bytes,
                       void *hip_stream);

/* The same stage through the PRODUCTION feature kernel (the instantiation salsa_extract_batch launches: packed-float32 pair solve
 * + float64 cold list, float32 output, or the float64 one under SALSA_FLAG_FORCE_F64): d_X as above, d_feat float32
 * [B][7][n_frames][n_bins] of which planes 4-6 are written (time-major, like salsa_extract_batch's output with F = n_bins; planes
 * 0-3 are not touched).  Exists so that the reference's extract_normalized_eigenvector goldens -- rank-1 windows, eigenvalue
 * ratios straddling cond_num, u[0] ~ 0, silence -- reach the solver that ships, not only salsa_eigvec_batch's float64 one. */
int salsa_eigvec_feature_batch(salsa_plan *plan, const float *d_X, int batch, int n_bins, int64_t n_frames, int lower_bin,
                               float *d_feat, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Schedule of salsa_extract_batch for the dataset scripts' main configuration (full SALSA, n_fft 512, n_hopframes 3, tracking on,
 * cond_num > 1; every other plan ignores the switch).  0: STFT -> tracker -> covariance / eigen, connected by the spectra spilled
 * to the workspace.  1 (round-5 stage a): STFT -> tracker as before, then ONE fused kernel that recomputes the STFT of a segment
 * of frames into a ring in LDS, rewrites the log-spectrogram and solves straight from the ring -- the spill is still written (the
 * tracker reads it) but no longer read back; it exists to measure the fused kernel against the two it replaces (measured:
 * slower, DESIGN.md section 6 -- the default stays 0).  2 (verification): as 1 with the deferred float64 records switched off,
 * i.e. every frame the packed solve hands back takes the fused kernel's in-step fallback.  Results are bit-identical in all three. */
int salsa_plan_set_fused(salsa_plan *plan, int mode);

/* Optional solver statistics (verification / study): d_counters = 4 device uint64, ADDED to by every covariance / eigen launch of
 * the plan: [0] work-list items (frame pairs), [1] gated frames in them, [2] frames handed to the float64 cold list (the packed
 * solve's `unsure` + small-pivot fallbacks), [3] tiles.  NULL (the default) detaches; the kernels then touch nothing. */
int salsa_plan_set_stats(salsa_plan *plan, unsigned long long *d_counters);

/* compute_scaler (salsa_feature_extraction.py:204-262) on device: accumulate float64 sum / sum-of-squares over time of
 * the first n_scaler_channels channels per frequency into d_sums [2][n_scaler_channels][n_freq] (zeroed by the caller
 * once; mean = sum/n, std = sqrt(sumsq/n - mean^2), population variance like sklearn's StandardScaler).  batch and
 * n_scaler_channels are grid dimensions of the one launch: above 65535 either is SALSA_EINVAL. */
int salsa_scaler_accumulate(const float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq,
                            int n_scaler_channels, double *d_sums, void *hip_stream);
/* normalise-on-load (dataset/database.py:197-202): d_feat[:, :n_scaler_channels] = (x - mean) / std in place;
 * d_mean / d_std float32 [n_scaler_channels][n_freq] (the scaler file's (4,1,F) arrays). */
int salsa_normalize_batch(float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq, int n_scaler_channels,
                          const float *d_mean, const float *d_std, void *hip_stream);

/* Fuse normalise-on-load into the extraction: with a scaler attached, salsa_extract_batch writes (x - mean) / std for the
 * 4 spectrogram channels (same float32 arithmetic as salsa_normalize_batch), saving the separate pass over the features.
 * d_mean / d_std: device float32 [4][F], caller-owned, must outlive the calls; (NULL, NULL) detaches. */
int salsa_plan_set_scaler(salsa_plan *plan, const float *d_mean, const float *d_std);

/* Feature rows [n_rows][n_frames][n_freq] float32 (time-major, what salsa_extract_batch writes; n_rows = batch * 7) ->
 * [n_rows][n_freq][n_frames] float64, the freq-major float64 array contrib/salsa_flexible.py returns (:264). */
int salsa_to_freq_major(const float *d_feat, int64_t n_rows, int64_t n_frames, int n_freq, double *d_out, void *hip_stream);

/* Training augmentation of a feature batch in one pass (utilities/transforms.py via dataset/datamodule.py:45-52, :73-82):
 * channel swap (TfmapRandomSwapChannelFoa :365-437 / ...Mic :440-523), RandomShiftUpDownNp (:286-320), then the
 * CompositeCutout rectangles (:58-283).  d_out: float32 [B][7][T][F]; d_in: the same block, possibly a view with its own
 * batch / channel strides in elements (e.g. extractor output cropped in time; rows stay contiguous).  The random draws are the
 * caller's: d_params int32 [B][40] = m0..m3 (swap bits; MIC uses three), shift (0 = none), up, 0, 0, top[8], h[8], left[8],
 * w[8] (h or w = 0: no rectangle; later rectangles win); d_uval float32 [B][8] in [0,1) and d_minmax float32 [B][2] give the
 * fill value min + (max - min) * u of the first 7 - n_zero_channels rows (the last n_zero_channels rows get 0). */
#define SALSA_AUGMENT_NPAR 40
int salsa_augment_batch(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch,
                        int64_t n_frames, int n_freq, int audio_format, int n_zero_channels, const int *d_params,
                        const float *d_uval, const float *d_minmax, void *hip_stream);
/* The baseline GCC recipe (melspecgcc / linspecgcc, dataset/datamodule.py:83-100) in one pass: GccRandomSwapChannelMic
 * (transforms.py:526-618; only the FIRST set bit of m0..m2 acts on the features, some GCC rows are flipped along the lag axis),
 * RandomShiftUpDownNp(n_last_channels=6) on the four spectrogram rows, then the cutout rectangles with the last 6 rows zeroed.
 * d_out: float32 [B][10][T][F]; d_in, d_params, d_uval, d_minmax as salsa_augment_batch (m3 unused). */
int salsa_augment_gcc_batch(const float *d_in, int64_t in_batch_stride, int64_t in_channel_stride, float *d_out, int batch,
                            int64_t n_frames, int n_freq, const int *d_params, const float *d_uval, const float *d_minmax,
                            void *hip_stream);

/* One training batch straight from the feature bank (dataset/database.py:230-231's concatenated layout; SeldDataset.__getitem__,
 * dataset/dataloader.py:37-62, for B chunks at once): gather B windows of chunk_frames frames, augment them as salsa_augment_batch /
 * salsa_augment_gcc_batch would (the same per-element code: the results are equal bit for bit) and cut the label windows, with the
 * target half of the channel swap applied.  d_bank: float32 [n_channels][bank_frames][n_freq], n_channels 7 or 10; d_sed_all float32
 * [label_frames_total][n_classes], d_doa_all float32 [label_frames_total][3 n_classes]; d_start / d_gt_start: int64 [batch], the first
 * feature frame / label frame of every chunk (0 <= start <= bank_frames - chunk_frames: the caller checks them; a window outside
 * the bank is left unwritten); recipe: SALSA_BANK_* (foa / mic: 7 channels, the last n_zero_channels of them zero-filled by the
 * cutout; gcc: 10 channels); d_params / d_uval as salsa_augment_batch takes them (NULL for SALSA_BANK_NONE).  has_rects != 0 (the
 * host drew at least one rectangle in the batch): the fill range, min / max of every UNAUGMENTED chunk, is first computed into
 * d_minmax_ws (8 bytes per sample, contents private); with has_rects == 0 that launch is skipped and d_minmax_ws may be NULL.
 * Outputs: d_x float32 [batch][n_channels][chunk_frames][n_freq], d_sed [batch][label_frames][n_classes], d_doa
 * [batch][label_frames][3 n_classes].  All five label arguments NULL: features only (whole clips with SALSA_BANK_NONE).  At most
 * three launches on hip_stream, no synchronisation; bank offsets are 64-bit. */
enum { SALSA_BANK_NONE = 0, SALSA_BANK_FOA = 1, SALSA_BANK_MIC = 2, SALSA_BANK_GCC = 3 };
int salsa_bank_batch(const float *d_bank, int n_channels, int64_t bank_frames, int n_freq, const float *d_sed_all,
                     const float *d_doa_all, int64_t label_frames_total, int n_classes, const int64_t *d_start,
                     const int64_t *d_gt_start, int batch, int chunk_frames, int label_frames, int recipe, int n_zero_channels,
                     const int *d_params, const float *d_uval, int has_rects, float *d_x, float *d_sed, float *d_doa,
                     void *d_minmax_ws, void *hip_stream);

/* Per-kernel timing of salsa_extract_batch with HIP events recorded on the call's stream (for roofline reporting).
 * enable == 1 brackets each launch with an event pair.  enable = K > 1 launches every kernel of the call K times back to
 * back between ONE event pair (each kernel is idempotent on the audio / spill / mask buffers, so the results are those of
 * a plain call) and reports elapsed / K: the per-launch average without an event between launches, which is what a
 * rocprofv3 kernel trace of the plain call shows (an event pair around a single launch inflates it by ~12 %).
 * enable = -1 / -2 (measurement only, no events): salsa_extract_batch issues only a PREFIX of the path -- the STFT launch
 * alone / STFT + tracker -- on the buffers a full call left behind, so a caller can time prefixes of the real launch
 * sequence with its own clock and attribute the step to its kernels by differences that add up to the step exactly.
 * Such a call returns SALSA_PARTIAL (1), not SALSA_OK: its outputs are incomplete and no caller can mistake it for a plain
 * call.  The mode persists on the plan until salsa_plan_set_timing(plan, >= 0).
 * salsa_plan_read_timing synchronises on the events and returns the milliseconds per launch of the last call's kernels
 * in issue order (n_out <= SALSA_MAX_KERNELS) and their names. */
#define SALSA_MAX_KERNELS 32
int salsa_plan_set_timing(salsa_plan *plan, int enable);
int salsa_plan_read_timing(salsa_plan *plan, float *ms, const char **names, int *n_out);

/* Pipelined schedule of salsa_extract_batch (default: n_groups 1, flags 0 = three kernels in order on the caller's stream).
 * n_groups > 1 (at most 16, capped at the batch size): the batch is cut into clip ranges whose kernels run on plan-owned
 * streams forked from / joined to the caller's stream, so the latency-bound noise-floor tracker of one group overlaps the
 * STFT / eigen kernels of the others.  SALSA_PIPE_SPLIT_PAIRS: the STFT of a group is two launches (channels 0/1, then 2/3)
 * and the tracker, which only needs channel 0, starts after the first.  SALSA_PIPE_GRAPH: the fork/join is captured once per
 * (buffers, sizes) into a plan-owned hipGraph and every later call with the same arguments is ONE hipGraphLaunch on the
 * caller's stream (a call made while the caller's stream is itself being captured issues the fork/join eagerly, so it
 * becomes part of the caller's graph).  Results are bit-identical under every schedule.  salsa_plan_set_groups(n) keeps
 * the current flags. */
enum { SALSA_PIPE_SPLIT_PAIRS = 1, SALSA_PIPE_GRAPH = 2 };
int salsa_plan_set_pipeline(salsa_plan *plan, int n_groups, int flags);
int salsa_plan_set_groups(salsa_plan *plan, int n_groups);

/* contrib/salsa_flexible.py accepts any number of microphones (stacked_covmat_eigh :52-77).  Up to 4 go through
 * salsa_extract_batch (fewer than 4: pad with silent channels).  5 - SALSA_MAX_MICS go through this entry point: plan created
 * with SALSA_FLAG_FLEX (SALSA or SALSA-Lite, MIC), d_audio float32 planar [B][n_channels][N] with n_channels EVEN, 6 .. 16 (an
 * odd count: append one silent channel -- the covariance only gains a zero eigenvalue -- and drop its output planes),
 * d_out float32 [B][2*n_channels - 1][T][F]: n_channels log-spectrograms, then n_channels - 1 spatial planes.  The
 * N x N eigenproblem is solved by cyclic complex Jacobi in float64, one lane per gated TF bin (6 and 8 channels: fully
 * unrolled instantiations; 10 - 16: one instantiation with the channel count read at run time). */
#define SALSA_MAX_MICS 16
size_t salsa_multichannel_workspace_bytes(const salsa_plan *plan, int n_channels, int batch, int64_t n_samples);
int salsa_extract_multichannel(salsa_plan *plan, const float *d_audio, int n_channels, int batch, int64_t n_samples,
                               float *d_out, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Diagnostic: the kernels' float32 dB conversion 10*log10(max(1e-10, p)) (librosa.power_to_db(ref=1, amin=1e-10, top_db=None),
 * salsa_feature_extraction.py:194-195) applied elementwise to d_power[n] -> d_db[n].  It is the SAME device function the STFT
 * kernel inlines (hardware v_log_f32 times a constant); exported so a test can bound its error over the whole float32
 * exponent range instead of over whatever dynamic range a test clip happens to have. */
int salsa_selftest_decibel(const float *d_power, float *d_db, int64_t n, void *hip_stream);

/* The resampling step of the reference's loader: librosa.load(path, sr=fs, mono=False, dtype=float32)
 * (dataset/salsa_feature_extraction.py:353, salsa_lite_feature_extraction.py:93) on a file whose native rate is not fs ->
 * librosa 0.8.0 core/audio.py::resample(res_type='kaiser_best', fix=True) -> resampy 0.2.2 (requirements.yml:181)
 * resample / interpn.py::resample_f.  d_x: float32 [n_rows][n_in] (one row per channel of a clip); d_y: float32
 * [n_rows][n_out_fixed]: n_out = int(n_in * sample_ratio) samples computed (each tap float32(float64(y) + weight * x), left
 * wing then right wing: the sequential reference loop bit for bit), then zeros up to n_out_fixed = ceil(n_in * sample_ratio)
 * (librosa's fix_length).  d_interp_win / d_interp_delta: float64 [n_win], the filter half-window (scaled by sample_ratio when
 * < 1) and its first differences; num_table: table entries per zero crossing (512 for kaiser_best); d_time_register: float64
 * [n_out], the reference's sequentially accumulated read positions (0, 1/ratio, 1/ratio + 1/ratio, ...).  salsa_amd/resample.py
 * builds all three. */
int salsa_resample_batch(const float *d_x, int n_rows, int64_t n_in, float *d_y, int64_t n_out, int64_t n_out_fixed, double sample_ratio,
                         const double *d_interp_win, const double *d_interp_delta, int n_win, int num_table,
                         const double *d_time_register, void *hip_stream);

/* The sample conversion inside librosa.load(path, sr=fs, mono=False, dtype=float32) (dataset/salsa_feature_extraction.py:353, lite :93:
 * soundfile reads the WAV's interleaved PCM frames as float32, librosa transposes to (channels, samples)).  d_pcm: the file's data chunk as
 * it is on disk, [n_frames][n_channels] samples of `sample_format`, aligned to one frame; d_out: float32 [n_channels][n_frames] (what
 * salsa_extract_batch takes as one planar clip).  int16 / 2^15, int32 / 2^31, (uint8 - 128) / 2^7, float32 as is: libsndfile's normalisation,
 * exact in float32.  Lets a loader upload raw file bytes (half the PCIe traffic for 16-bit clips) and do no arithmetic on the host. */
#define SALSA_PCM_S16 1
#define SALSA_PCM_S32 2
#define SALSA_PCM_U8 3
#define SALSA_PCM_F32 4
int salsa_pcm_to_planar(const void *d_pcm, int sample_format, int n_channels, int64_t n_frames, float *d_out, void *hip_stream);

/* Labelled scenes rendered on the device (salsa_amd/scenes.py; the reference has no counterpart: the definition is
 * this project's).  A clip is a list of items (event, response, onset, gain):
 *     audio[b, c, n] = ambient[b, c, n] + sum_i gain_i (h[rir_i, c, :] * event_i)[n - onset_i],   0 <= n < n_samples,
 * `*` the full linear convolution, evaluated in float32 by overlap-save on partitions of 512 samples.  A sample outside every item's
 * support [onset, onset + length + rir_len - 1) is the ambient's value bit for bit (zero without ambient); two calls give equal bits, and
 * a clip's result does not depend on the other clips of the call.
 *
 * salsa_scene_rir_spectra: d_rirs float32 [n_rirs][n_channels][rir_len] -> the partition spectra, in a 16-byte aligned buffer of
 * salsa_scene_rir_spectra_bytes (8192 bytes of transform constants, then ceil(rir_len / 512) x 4096 bytes per response and channel).
 * Once per bank.  Limits: 1 <= n_channels <= 16, 1 <= rir_len <= 16384.
 *
 * salsa_scene_render: d_events float32 [n_event_samples], the pool's signals one behind the other.  The item tables are given twice,
 * with equal contents: on the HOST (clip_start, items, gains), where every entry is checked before the first device call, and on the
 * device (d_clip_start, d_items, d_gains), where the kernels read them.  clip_start int [n_clips + 1]: clip b owns items clip_start[b]
 * .. clip_start[b + 1] - 1, at most 256 of them, rendered in that order; items int64 [4][n_items]: the event's first sample in
 * d_events, the onset in the clip (0 <= onset < n_samples, any value: no alignment), the event's length (1 .. max_event_len) and the
 * response's index; gains float32 [n_items].  d_ambient: float32 [n_clips][n_channels][n_samples] or NULL (may be d_out); d_out the
 * same shape.  d_workspace: 16-byte aligned, salsa_scene_workspace_bytes(n_samples, max_event_len, n_items) = n_items x min(
 * (max_event_len + 510) / 512 + 2, ceil(n_samples / 512)) x 4096 bytes; not needed for n_items = 0.  Two launches on hip_stream, whatever
 * n_clips and n_items are.  Returns -1 for an argument outside these limits or tables that contradict each other, -5 for a workspace
 * too small; the two size queries return 0 for arguments the calls would refuse. */
size_t salsa_scene_rir_spectra_bytes(int n_rirs, int n_channels, int rir_len);
int salsa_scene_rir_spectra(const float *d_rirs, int n_rirs, int n_channels, int rir_len, float *d_spectra, void *hip_stream);
size_t salsa_scene_workspace_bytes(int64_t n_samples, int max_event_len, int n_items);
int salsa_scene_render(const float *d_events, int64_t n_event_samples, const float *d_rir_spectra, int n_rirs, int n_channels, int rir_len,
                       const int *clip_start, const int64_t *items, const float *gains, const int *d_clip_start, const int64_t *d_items,
                       const float *d_gains, int n_clips, int n_items, int max_event_len, const float *d_ambient, float *d_out,
                       int64_t n_samples, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* Moving sources.  An item with a trajectory of responses, one node every S samples of its dry time, is cut by
 * the caller into SEGMENTS, one per node: node k covers the dry samples ((k - 1) S, (k + 1) S) of the event, weighted by the window
 * (float)(S - |n - k S|) / (float)S, the windowed sample rounded once, and convolved with node k's response; the windows of neighbouring
 * nodes sum to one, so the input is cross-faded linearly from response to response.  The call renders
 *     audio[b, c, n] = ambient[b, c, n] + sum_s gain_s (h[rir_s, c, :] * (w_s . x_s))[n - onset_s],   0 <= n < n_samples,
 * over the segments s of clip b, with the properties of salsa_scene_render (the ambient's bits outside every segment's support
 * [onset, onset + length + rir_len - 1), equal bits from two calls, a clip independent of its batch, two launches on hip_stream,
 * nothing allocated or synchronised).  A segment of step 0 has no window: a static item is ONE such segment, and a call whose segments
 * are all of that kind gives the bits of salsa_scene_render on the same items.
 *
 * The tables are given twice with equal contents, on the host (checked entry by entry before the first device call) and on the device.
 * clip_start int [n_clips + 1] (host only): clip b owns segments clip_start[b] .. clip_start[b + 1] - 1, at most 65536 of them,
 * accumulated in that order.  segments int64 [6][n_segments]: the segment's first sample in d_events, its onset in the clip (0 <= onset
 * < n_samples: the item's onset plus the segment's start in the event; a segment that would start at or past n_samples is left out by
 * the caller), its length (1 .. max_segment_len), the response's index, the ramp's centre counted from the segment's first sample, and
 * the ramp step S: 0 (no window) or 240 .. 16777216, with |q - centre| < S for every sample 0 <= q < length, so that no weight is zero
 * or negative.  gains float32 [n_segments].  block_table int [n_clips][ceil(n_samples / 512)][2]: for output block m of clip b (samples
 * [512 m, 512 m + 512)) the first and the one-past-last segment the render kernel visits; it visits only these, so the range must hold
 * every segment of the clip that reaches the block, i.e. with onset / 512 <= m <= min((onset + length - 1) / 512 + 1, M - 1) +
 * ceil(rir_len / 512) - 1, and lie inside the clip's segments.  The host checks that no reaching segment is left out.
 * d_workspace: 16-byte aligned, salsa_scene_moving_workspace_bytes(n_samples, max_segment_len, n_segments) = n_segments x min(
 * (max_segment_len + 510) / 512 + 2, ceil(n_samples / 512)) x 4096 bytes: sized by the longest SEGMENT (2 S - 1 samples when every
 * item moves), not by the longest event; not needed for n_segments = 0 (the block table is).  Limits on channels, response length and
 * clips as above.  Returns -1 for an argument outside these limits or tables that contradict each other, -5 for a workspace too
 * small; the size query returns 0 for arguments the call would refuse. */
size_t salsa_scene_moving_workspace_bytes(int64_t n_samples, int max_segment_len, int n_segments);
int salsa_scene_render_moving(const float *d_events, int64_t n_event_samples, const float *d_rir_spectra, int n_rirs, int n_channels,
                              int rir_len, const int *clip_start, const int64_t *segments, const float *gains, const int *block_table,
                              const int64_t *d_segments, const float *d_gains, const int *d_block_table, int n_clips, int n_segments,
                              int max_segment_len, const float *d_ambient, float *d_out, int64_t n_samples, void *d_workspace,
                              size_t workspace_bytes, void *hip_stream);

/* Spatially diffuse ambient noise (salsa_amd/ambient.py; the reference has no counterpart: the definition is this
 * project's).  n_dirs uncorrelated plane-wave noises reach the four channels through the array's direct-path response, one colouring
 * filter follows, and the result is added to the rendered audio at a per-clip scale:
 *     m[c][t] = sum_{d < n_dirs} sum_{k < mix_taps} mix[d][c][k] white(seed_b, d, t - k)
 *     y[c][n] = sum_{j < colour_taps} colour[j] m[c][n - j]
 *     out[b][c][n] = fmaf(scale_b, y[c][n], in[b][c][n]),   without d_in: scale_b * y[c][n],   0 <= n < n_samples,
 * all float32 fmaf chains from +0.0 in the order written (d outer, k inner, j, each ascending).  white(seed, d, n) is a counter hash, a
 * pure function of its three integers defined from n = -1024 on (so the noise has no onset at sample 0), mean 0 and variance 1; it is
 * stated in salsa_amd/csrc/scene_diffuse.hip's header and restated in tests/diffuse_reference.py.
 * d_mix float32 [n_dirs][n_channels][mix_taps], d_colour float32 [colour_taps], d_seeds uint64 [n_clips], d_scales float32 [n_clips] --
 * all on the device, so a scale computed there needs no synchronisation.  d_in float32 [n_clips][n_channels][n_samples] or NULL, and it
 * may be d_out; d_out the same shape.  A clip whose scale is 0 gets d_in's bits (+0.0 without d_in).  A clip's bits depend on its seed,
 * its scale and its input alone -- not on the batch, its place in it or n_samples (a shorter call gives the first samples' bits) --, and
 * two calls give equal bits.  One launch on hip_stream, nothing allocated or synchronised; a workgroup owns
 * salsa_scene_diffuse_block() = 2048 consecutive samples of one clip.
 * Supported (salsa_scene_diffuse_supported, host only, 1 or 0): n_channels == 4, 1 <= n_dirs <= 256, 1 <= mix_taps <= 128, 1 <=
 * colour_taps <= 513 and odd.  Further n_clips >= 1, 1 <= n_samples < 2^32 and at most 2^31 - 1 blocks in all.  Returns -1 for a shape
 * outside these limits or a null pointer, before any device call, and -6 when the launch fails. */
int salsa_scene_diffuse_block(void);
int salsa_scene_diffuse_supported(int n_channels, int n_dirs, int mix_taps, int colour_taps);
int salsa_scene_diffuse(const float *d_mix, int n_dirs, int n_channels, int mix_taps, const float *d_colour, int colour_taps,
                        const uint64_t *d_seeds, const float *d_scales, const float *d_in, float *d_out, int n_clips, int64_t n_samples,
                        void *hip_stream);

/* Shoebox room responses by the image-source method (salsa_amd/rooms.py; the reference has no counterpart: the
 * definition is this project's).  The caller has enumerated the room's images once, for all sources: image i mirrors a source s to
 * p = sign_i o s + shift_i (sign = 1 - 2 q, shift = 2 n o L) with the amplitude A_i (the walls' reflection coefficients to the powers
 * of their reflection counts; the order limit already applied).  For source r and receiver point rho:
 *     d = |p - rho|,  tau = d fs_over_c - t0_r,  out[r, c, k] += g_r (A_i / d) gain_c w(k - tau),   0 <= k < rir_len,
 * w(x) = sinc(x) (1 + cos(pi x / 16)) / 2 for |x| < 16 and 0 otherwise.  SALSA_ROOM_OMNI: channel c is receiver c, gain 1.
 * SALSA_ROOM_FOA: ONE receiver, four channels W, Y, Z, X with the gains (1, u_y, u_z, u_x), u = (p - rho) / d.  Positions, distances,
 * delays and the fractional part of tau are float64; from the tap argument on the arithmetic is float32, each tap summed over the
 * images in TABLE ORDER: two calls give equal bits, a source's response does not depend on the other sources of the call, and a tap
 * that no image's support reaches is +0.0.  Every element of out is written.
 *
 * The tables are given twice with equal contents, on the host (checked entry by entry before the first device call) and on the device.
 * images double [7][n_images]: the rows sign x, y, z (each +1 or -1), shift x, y, z, amplitude (0 < A <= 1); 1 <= n_images <=
 * salsa_room_max_images() = 4194304.  sources double [n_sources][5]: position x, y, z, the time origin t0 (a whole number >= 0) and the
 * gain g > 0; 1 <= n_sources <= 65535.  receivers double [n_receivers][3], HOST only, 1 .. 4 of them.  1 <= rir_len <= 16384.
 * d_out float32 [n_sources][C][rir_len], C = n_receivers (omni) or 4 (FOA).  One launch on hip_stream, nothing allocated or
 * synchronised; a workgroup owns salsa_room_tap_block() = 256 consecutive taps of one (source, receiver).  Returns -1 for a null
 * pointer or an argument outside these limits, before any device call; -6 when the launch fails. */
#define SALSA_ROOM_OMNI 0
#define SALSA_ROOM_FOA 1
int salsa_room_max_images(void);
int salsa_room_tap_block(void);
int salsa_room_rirs(const double *images, const double *d_images, int n_images, const double *sources, const double *d_sources,
                    int n_sources, const double *receivers, int n_receivers, int mode, double fs_over_c, int rir_len, float *d_out,
                    void *hip_stream);

/* The MIC capsules of a shoebox room on a RIGID sphere (salsa_amd/rooms.py: baffle='rigid'; the reference has no
 * counterpart: the definition is this project's).  The pressure of a plane wave from the unit direction u at a capsule at the unit
 * direction m on a rigid sphere of radius R, relative to the free-field pressure at the sphere's centre, is the series
 *     H(f, Theta) = sum_{n=0}^{N} i^n (2 n + 1) b_n(k R) P_n(cos Theta),   b_n(x) = j_n(x) - j_n'(x) / h_n^(2)'(x) h_n^(2)(x),
 *     k = 2 pi f / c,  cos Theta = u . m,  H(0, Theta) = 1.
 * The host (salsa_amd/rooms.py: SphereTable) turns it into a float32 table S[Q + 1][P + 1][lead + trail] of band-limited tap weights:
 * S[q][p][j] = h_{q pi / Q}(j - (lead - 1) - p / P), h_Theta(x) = sum_n a_Theta[n] w(x - n), a_Theta the inverse real FFT of H times a
 * raised-cosine taper, cut to a fixed support, w the Hann-windowed sinc of salsa_room_rirs; row P is row 0 one tap on.  This call only
 * READS the table.  For source r, image i and capsule m, with d and tau measured to the array CENTRE (one distance and one delay for
 * all four capsules: a far-field, plane-wave model),
 *     v = sign_i o s_r + shift_i - centre,  d = |v|,  tau = d fs_over_c - t0_r,  k0 = floor(tau),  fr = tau - k0,
 *     cos Theta_m = clamp((v . unit_m) / d, -1, 1),  qf = acos(cos Theta_m) Q / pi,  q = min(floor(qf), Q - 1),  wq = qf - q,
 *     pf = fr P,  p = min(floor(pf), P - 1),  wp = pf - p,  j = k - k0 + lead - 1,
 *     out[r, m, k] += g_r (A_i / d) ((1 - wq) ((1 - wp) S[q][p][j] + wp S[q][p + 1][j]) + wq ((1 - wp) S[q + 1][p][j] + wp S[q + 1][p + 1][j]))
 * for 0 <= j < lead + trail and 0 <= k < rir_len: the image's taps are k0 - lead + 1 .. k0 + trail.  Theta = pi reads the rows Q - 1 and
 * Q with the weights (0, 1), and no fraction reads a phase row past P.  Everything up to k0, fr, wq, wp and the coefficient g A / d is
 * float64, each rounded once; from the table lookup on the arithmetic is float32, each tap summed over the images in TABLE ORDER: two
 * calls give equal bits, a source's response does not depend on the other sources of the call, a capsule's row does not depend on
 * the other capsules' directions, and a tap that no image's support reaches is +0.0.  Every element of out is written.
 *
 * images, sources (and their device copies) as for salsa_room_rirs.  centre double [3] and capsule_units double [4][3], HOST only, each
 * unit of length 1 to within 1e-6.  table / d_table float32 [Q + 1][P + 1][lead + trail], host and device with equal contents; the
 * host copy is checked entry by entry (finite) before the first device call.  salsa_room_sphere_limits writes the largest Q, P and
 * lead + trail (4096, 1024, 512; each pointer may be NULL) and returns the largest number of table entries, 1 << 27.  1 <= Q, 1 <= P,
 * 1 <= lead, 1 <= trail.  d_out float32 [n_sources][4][rir_len].  A source or an image AT the centre (d = 0) is the caller's to
 * exclude.  One launch on hip_stream, nothing allocated or synchronised; a workgroup owns salsa_room_tap_block() = 256 consecutive
 * taps of one source and all four capsules.  Returns -1 for a null pointer or an argument outside these limits, before any device
 * call; -6 when the launch fails. */
int salsa_room_sphere_limits(int *max_q, int *max_p, int *max_support);
int salsa_room_rirs_sphere(const double *images, const double *d_images, int n_images, const double *sources, const double *d_sources,
                           int n_sources, const double *centre, const double *capsule_units, const float *table, const float *d_table,
                           int Q, int P, int lead, int trail, double fs_over_c, int rir_len, float *d_out, void *hip_stream);

/* Energy decay and room-acoustic parameters of a bank of impulse responses (salsa_amd/rooms.py: rir_acoustics, calibrate_room;
 * DESIGN.md section 9n; the reference has no counterpart: the definition is this project's).  d_rirs float32 [n_rirs][n_channels]
 * [rir_len], finite.  Per (response, channel), in float64 throughout:
 *     e[n] = h[n]^2,  EDC[n] = sum_{m >= n} e[m] (Schroeder's backward integral),  E = EDC[0],  n_d = the FIRST index of the largest |h|,
 *     i(x) = the first n with EDC[n] <= E 10^(x / 10), decided on energies with the host's five factors (x = 0, -5, -10, -25, -35 dB),
 *     EDT, T20, T30 = -60 / slope of the least-squares line through (n / fs, 10 log10(EDC[n] / E)) over n in [i(lo), i(hi)], both
 *         included, (lo, hi) = (0, -10), (-5, -25), (-5, -35) dB, centred sums; NaN when i(hi) does not exist, EDC[i(hi)] = 0 or the
 *         range has fewer than two points,
 *     headroom = -(slope per tap) (rir_len - 1 - i(hi)) dB: the decay the fitted line predicts between the range's end and the cut,
 *     DRR = 10 log10(E_dir / E_rest): the taps within direct_halfwidth of n_d against all others (+inf when E_rest = 0),
 *     C50 = 10 log10(E_early / E_late): the taps n < n_d + round(0.05 fs) against the others (+inf when E_late = 0).
 * A silent response (E = 0) has energy 0, peak 0 and NaN everywhere else; its curve is 0.  d_params double [n_rirs][n_channels]
 * [SALSA_DECAY_PARAMS], indexed by the enum below (the crossings as whole numbers, NaN where there is none); d_edc double [n_rirs]
 * [n_channels][rir_len] receives the curve, or NULL: the parameters' bits are the same either way.  One launch on hip_stream, one
 * workgroup per (response, channel), no atomics, every sum in a fixed order: two calls give equal bits and a response's result does
 * not depend on the rest of the batch.  Nothing is allocated or synchronised.  1 <= n_rirs <= 65535, 1 <= n_channels <= 16, 1 <=
 * rir_len <= 16384, 0 < fs <= 1e9, 0 <= direct_halfwidth <= 16384.  Returns -1 for a null pointer or an argument outside these
 * limits, before any device call; -6 when the launch fails. */
enum {
    SALSA_DECAY_ENERGY = 0,
    SALSA_DECAY_PEAK = 1,
    SALSA_DECAY_EDT = 2,
    SALSA_DECAY_T20 = 3,
    SALSA_DECAY_T30 = 4,
    SALSA_DECAY_HEADROOM_EDT = 5,
    SALSA_DECAY_HEADROOM_T20 = 6,
    SALSA_DECAY_HEADROOM_T30 = 7,
    SALSA_DECAY_DRR_DB = 8,
    SALSA_DECAY_C50_DB = 9,
    SALSA_DECAY_CROSS_0DB = 10,
    SALSA_DECAY_CROSS_5DB = 11,
    SALSA_DECAY_CROSS_10DB = 12,
    SALSA_DECAY_CROSS_25DB = 13,
    SALSA_DECAY_CROSS_35DB = 14,
    SALSA_DECAY_PARAMS = 15
};
int salsa_rir_decay_params(void);
int salsa_rir_decay(const float *d_rirs, int n_rirs, int n_channels, int rir_len, double fs, int direct_halfwidth, double *d_params,
                    double *d_edc, void *hip_stream);

/* Shoebox rooms whose walls differ per octave band (salsa_amd/rooms.py: ShoeboxRoom(bands=...); the reference has
 * no counterpart: the definition is this project's).  A banded room has K amplitude rows over ONE image table, and K linear-phase
 * filters h_b of 2 half + 1 taps, centre `half`, that sum to a unit impulse at `half` (rooms.octave_filters).  With r_b the response
 * of salsa_room_rirs for the amplitude row of band b, evaluated on the taps -half .. L + half - 1, the banded response is
 *     h[s, c, k] = sum_b sum_{j = 0}^{2 half} h_b[j] r_b[s, c, k + half - j],   0 <= k < L,
 * and the band signals of a measured response x (zero outside [0, L)) are y_b[k] = sum_j h_b[j] x[k + half - j].
 *
 * salsa_room_rirs_bands: the r_b.  images double [6 + K][n_images]: the rows sign x, y, z, shift x, y, z of salsa_room_rirs, then one
 * amplitude row per band, 0 <= A <= 1 (a band may be 0 where another is not); 1 <= K <= salsa_room_max_bands() = 8.  sources,
 * receivers, mode and fs_over_c as for salsa_room_rirs.  The taps are first_tap .. first_tap + n_taps - 1, |first_tap| <= 4096 and 1 <=
 * n_taps <= 16384 + 4096; d_out float32 [n_sources][C][K][n_taps], element t the tap first_tap + t.  An image's float64 geometry, its
 * delay, fraction and windowed sinc are computed once and applied to K accumulators with K coefficients g A_b / d (times u_c), each
 * formed in float64 and rounded once.  As for salsa_room_rirs: table-order sums without atomics, equal bits from two calls, a source
 * independent of its batch, +0.0 where no support reaches, every element written; and a tap's bits depend neither on first_tap nor
 * on n_taps.  With K = 1, first_tap = 0 and amplitudes > 0 the output is salsa_room_rirs's bit for bit.
 *
 * salsa_band_merge: d_bands float32 [n][K][L + 2 half] (element e of a row is tap e - half), d_filters float32 [K][2 half + 1] ->
 * d_out float32 [n][L], the first sum.  salsa_band_split: d_x float32 [n][L] -> d_out float32 [n][K][L], the second.  Both run in
 * float32, every output ONE chain acc = fma(h_b[j], x_b[k + half - j], acc) from +0.0, b ascending outside (merge), j ascending inside,
 * a zero for an input outside its row: two calls give equal bits, a row does not depend on its batch, and an impulse in gives the
 * filter's taps bit for bit.  Inputs are finite.  1 <= n <= 1048576, 1 <= L <= 16384, 1 <= half <= 2048.  A workgroup owns 2048
 * outputs of a row (direct form from LDS).  One launch per 65535 rows on hip_stream, nothing allocated or synchronised.
 * All three return -1 for a null pointer or an argument outside these limits, before any device call; -6 when a launch fails. */
int salsa_room_max_bands(void);
int salsa_room_rirs_bands(const double *images, const double *d_images, int n_images, int n_bands, const double *sources,
                          const double *d_sources, int n_sources, const double *receivers, int n_receivers, int mode, double fs_over_c,
                          int first_tap, int n_taps, float *d_out, void *hip_stream);
int salsa_band_merge(const float *d_bands, const float *d_filters, int n, int n_bands, int length, int half, float *d_out,
                     void *hip_stream);
int salsa_band_split(const float *d_x, const float *d_filters, int n, int n_bands, int length, int half, float *d_out, void *hip_stream);

/* Sources localised from the features' directional channels by a DOA histogram (salsa_amd/localize.py; the
 * reference has no counterpart: the definition is this project's).  d_feat float32 [batch][n_channels >= 7][n_frames][n_freq], time-major
 * as salsa_extract_batch writes it; only the columns [col0, col1) of the channels 4 - 6 are read.  frames_per_label = P feature frames
 * make one label frame, Fl = n_frames / P of them (trailing frames are ignored).  The votes of label frame f are the cells (t, col),
 * P f <= t < P (f + 1), t ascending, then col ascending:
 *     v = (ch4, ch5, ch6)[t][col]; no vote when all three are zero (either sign) or one is not finite
 *     FOA: u = (v[2], v[0], v[1]) (the channels are Y, Z, X);  MIC: u_i = fmaf(M[i][2], v[2], fmaf(M[i][1], v[1], M[i][0] v[0])),
 *         M = mic_matrix, HOST float32 [3][3], the inverse of the rows p_m - p_0 of the capsule positions (NULL for FOA)
 *     n = sqrtf(fmaf(u_z, u_z, fmaf(u_y, u_y, u_x u_x))); no vote unless norm_lo <= n <= norm_hi; u = u / n
 * The grid is equal-angle with a step of grid_step degrees (it divides 90, 3 .. 30): elevation -90 .. 90, each pole ONE cell, elsewhere
 * the azimuths -180 .. 180 - step, numbered elevation-major: salsa_doa_hist_cells(step) = (360 / step)(180 / step - 1) + 2 cells (0 for a
 * step not taken).  d_grid float32 [cells][3] holds their unit vectors (x, y, z), the caller's table.
 *     score[g] = sum over the votes, in vote order, of max(0, (dot(u, U[g]) - cos_kernel) inv_kernel),
 *     dot(u, U) = fmaf(u_z, U_z, fmaf(u_y, U_y, u_x U_x)),
 * float32 throughout, no transcendental.  Peaks, for k = 0 .. max_sources - 1: g* is the unsuppressed cell of greatest score, the lowest
 * index on a tie; stop when score[g*] < min_score; the refined direction is m / |m|, m the float32 sum in vote order of the votes with
 * dot(u, U[g*]) >= cos_kernel; then every cell with dot(U[g], U[g*]) >= cos_suppress is suppressed.
 * Outputs per (clip, label frame): d_count int32 [batch][Fl] the peaks found, d_votes int32 [batch][Fl] the votes cast, d_cell int32
 * [batch][Fl][K], d_score float32 [batch][Fl][K], d_direction float32 [batch][Fl][K][3] (x, y, z); unused slots hold -1, +0.0, +0.0.
 * d_spectrum float32 [batch][Fl][cells] or NULL: every cell's score, none suppressed; the other outputs' bits are the same either way.
 * One launch on hip_stream, one workgroup per label frame, no atomics, no scratch, nothing allocated or synchronised: two calls give
 * equal bits and a clip's result does not depend on its batch.
 * salsa_doa_hist_supported (host only, 1 or 0): n_channels >= 7, 0 <= col0 < col1 <= n_freq, P >= 1, P (col1 - col0) <= 4096, a step
 * taken, 1 <= max_sources <= 8.  salsa_doa_hist_limits writes the largest number of cells per label frame (4096), of sources (8) and
 * of grid cells (each pointer may be NULL) and returns the workgroup's size.  Further batch >= 1, Fl >= 1, batch Fl < 2^31, -1 <
 * cos_kernel < 1, inv_kernel > 0, -1 <= cos_suppress <= 0.9999 (a peak must suppress its own cell), min_score > 0, 0 < norm_lo <=
 * norm_hi finite.  Returns -1 for a null pointer or an argument outside these limits, before any device call; -6 when the launch fails. */
int salsa_doa_hist_limits(int *max_votes, int *max_sources, int *max_cells);
int salsa_doa_hist_cells(int grid_step);
int salsa_doa_hist_supported(int n_channels, int n_freq, int col0, int col1, int frames_per_label, int grid_step, int max_sources);
int salsa_doa_hist(const float *d_feat, int batch, int n_channels, int64_t n_frames, int n_freq, int col0, int col1,
                   int frames_per_label, int audio_format, const float *mic_matrix, const float *d_grid, int grid_step,
                   float cos_kernel, float inv_kernel, float cos_suppress, float min_score, float norm_lo, float norm_hi,
                   int max_sources, int *d_count, int *d_votes, int *d_cell, float *d_score, float *d_direction,
                   float *d_spectrum, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SALSA_HIP_H */
