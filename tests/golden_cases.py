"""Parameter-set cases of fixtures g19 (win_len != n_fft) and g20 (off-default settings), written by tools/make_golden.py
ref_case: per case the reference's extract_features settings, its clips (seed, length, rate, SHA-256), and per clip the
spatial channels whole ('<case>|<clip>|spatial') and the spectrogram channels every `stride`-th frame ('<case>|<clip>|logspec')."""
import numpy as np

from salsa_amd.synth import sha256_of, synth_clip


def case_clips(c):
    """{clip name: (4, N) float32} regenerated from the seeds, checked against the clips the reference saw (sorted by name, as
    the reference lists its audio directory)."""
    out = {}
    for name in sorted(c['clips']):
        seed, n, fs, sha = c['clips'][name]
        y = synth_clip(seed, n, fs=fs)
        assert sha256_of(y) == sha, 'synthetic clip generator drifted from the golden fixtures (seed %d)' % seed
        out[name] = y
    return out


def oracle_features(oracle, c, y):
    """the oracle on one clip with the case's settings -> ((7, T, F) float32, gate margins (nd, T) or None)"""
    kw = dict(fs=c['fs'], n_fft=c['n_fft'], hop=c['hop'], win=c['win'], fmin_doa=c['fmin_doa'], fmax_doa=c['fmax_doa'])
    if c['kind'] == 'salsa':
        out, aux = oracle.extract_salsa(y, cond_num=c['cond_num'], n_hopframes=c['n_hopframes'], audio_format=c['format'],
                                        return_aux=True, **kw)
        return out, aux['margin']
    return oracle.extract_lite(y, feature_type=c['kind'], **kw), None


def extractor_kwargs(c):
    """SalsaExtractor arguments of the case (the YAML data block + extract_features' arguments)"""
    return dict(fs=c['fs'], n_fft=c['n_fft'], hop_len=c['hop'], win_len=c['win'], fmin_doa=c['fmin_doa'], fmax_doa=c['fmax_doa'],
                cond_num=c['cond_num'], n_hopframes=c['n_hopframes'], audio_format=c['format'], feature_type=c['kind'])


def lite_period(c, lower, F):
    """one phase turn of each SALSA-Lite / IPD feature row (bins lower .. lower+F-1): 2 for IPD (angle / pi), 2 pi / (delta k)
    for SALSA-Lite (salsa_lite_feature_extraction.py:62-65, :113-115)"""
    if c['kind'] == 'salsa_ipd':
        return 2.0 * np.ones(F)
    k = np.arange(lower, lower + F, dtype=np.float64)
    return 2 * np.pi / (2 * np.pi * c['fs'] / (c['n_fft'] * 343.0) * k)


def mirror_frames(n, hop):
    """frames whose samples are mirror-symmetric about a reflect point (real spectra up to round-off): frame 0, and the last
    frame when (n - 1) % hop == 0"""
    T = 1 + n // hop
    return [0] + ([T - 1] if (n - 1) % hop == 0 else [])
