/*
 * salsa_baseline.h -- C ABI of the baseline SELD features in libsalsa_hip.so: log-mel / log-linear spectrograms with the
 * intensity vector (FOA) or GCC-PHAT (MIC), the inputs the SALSA papers compare against.
 *
 *   reference interface (file:line, relative to the upstream repo)                 replaced by
 *   -----------------------------------------------------------------------------  ----------------------------------------
 *   MelSpecExtractor.extract, dataset/feature_extraction.py:224-267                salsa_baseline_extract_batch (MELSPEC)
 *   MelSpecIvExtractor.extract, dataset/feature_extraction.py:159-221              salsa_baseline_extract_batch (MELSPECIV)
 *   MelSpecGccExtractor.extract / gcc_phat / logmel, :54-156                       salsa_baseline_extract_batch (MELSPECGCC)
 *   LinSpecIvExtractor.extract, dataset/feature_extraction.py:270-359              salsa_baseline_extract_batch (LINSPECIV)
 *   LogSpecGccExtractor.extract / gcc_phat / logspec, :362-483                     salsa_baseline_extract_batch (LINSPECGCC)
 *   FeatureExtractor.melW = librosa.filters.mel(...) (librosa 0.8.0), :45          salsa_baseline_mel_matrix (host)
 *   extract_features() n_mels / n_freqs and shapes, :629-645                        salsa_baseline_output_shape
 *   compute_scaler, dataset/feature_extraction.py:526-594                          salsa_scaler_accumulate (salsa_hip.h) or host sums
 *
 * Conventions are those of salsa_hip.h: 0 or a negative SALSA_E* code, the message in salsa_last_error(); device pointers
 * are caller-owned, work is enqueued on the caller's stream, and nothing is allocated or synchronised inside the extract
 * call (hipGraph-capturable).  A plan is bound to the device current at salsa_baseline_plan_create.
 *
 * Input: planar float32 audio [B][4][N].  Output: float32 [B][C][T][F] with T = 1 + N / hop_len and
 *   MELSPEC     C = 4   log-mel                                  F = n_mels
 *   MELSPECIV   C = 7   log-mel, IV x/y/z through melW           F = n_mels
 *   MELSPECGCC  C = 10  log-mel, GCC-PHAT of pairs (0,1),(0,2),(0,3),(1,2),(1,3),(2,3)   F = n_mels (kept lags)
 *   LINSPECIV   C = 7   log-linear, IV x/y/z through W           F = 200 | 100 (compressed) or n_fft/2
 *   LINSPECGCC  C = 10  log-linear, GCC-PHAT                     F = 200 | 100 or n_fft/2
 * n_fft must be 256 or 512 for every type (the reference's mel types accept others: not supported here, SALSA_ENFFT).
 * Clips of n_samples <= the reflect padding of the largest STFT the type runs (n_fft/2, or 2*n_fft/2 = n_fft for the GCC
 * types' 2*n_fft-point STFT) are refused with SALSA_EINVAL.
 */
#ifndef SALSA_BASELINE_H
#define SALSA_BASELINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SALSA_BASELINE_MELSPEC = 0,    /* 'melspec' */
    SALSA_BASELINE_MELSPECIV = 1,  /* 'melspeciv' */
    SALSA_BASELINE_MELSPECGCC = 2, /* 'melspecgcc' */
    SALSA_BASELINE_LINSPECIV = 3,  /* 'linspeciv' */
    SALSA_BASELINE_LINSPECGCC = 4  /* 'linspecgcc' */
};

typedef struct salsa_baseline_params {
    int fs;                 /* cfg['data']['fs'] */
    int n_fft;              /* 256 | 512 */
    int hop_len;
    int win_len;            /* <= n_fft; periodic Hann centred in the FFT frame */
    int n_mels;             /* mel types: mel bands (and kept GCC lags); ignored by the lin types */
    int feature_type;       /* SALSA_BASELINE_* */
    double fmin, fmax;      /* mel types: librosa.filters.mel's fmin / fmax in Hz (fmax <= 0: fs / 2), used as given:
                             * only extract_features (Python) clamps fmax to fs // 2, as the reference's extract_features does */
    int is_compressed_freq; /* lin types: 1 -> 200 | 100 rows (bins above 9 kHz in groups of 8), 0 -> n_fft / 2 rows */
    int reserved;           /* 0 */
} salsa_baseline_params;

typedef struct salsa_baseline_plan salsa_baseline_plan;

int salsa_baseline_plan_create(const salsa_baseline_params *params, salsa_baseline_plan **out_plan);
int salsa_baseline_plan_destroy(salsa_baseline_plan *plan);
/* (C, T, F) of one clip of n_samples samples per channel */
int salsa_baseline_output_shape(const salsa_baseline_plan *plan, int64_t n_samples, int *n_channels, int64_t *n_frames,
                                int *n_freq);
/* bytes of device workspace salsa_baseline_extract_batch needs (0 today: the kernels keep everything on chip) */
size_t salsa_baseline_workspace_bytes(const salsa_baseline_plan *plan, int batch, int64_t n_samples);
/* d_audio float32 [batch][4][n_samples] -> d_out float32 [batch][C][T][F]; one kernel launch per call */
int salsa_baseline_extract_batch(salsa_baseline_plan *plan, const float *d_audio, int batch, int64_t n_samples, float *d_out,
                                 void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* host: librosa.filters.mel(sr=fs, n_fft, n_mels, fmin, fmax) of librosa 0.8.0 (Slaney scale, norm='slaney') into
 * out[n_mels][n_fft/2 + 1] float32, in librosa's order of operations (fmax <= 0: fs / 2). */
int salsa_baseline_mel_matrix(int fs, int n_fft, int n_mels, double fmin, double fmax, float *out);

#ifdef __cplusplus
}
#endif

#endif /* SALSA_BASELINE_H */
