#!/usr/bin/env python
"""Golden vector g26: SALSA-Lite / SALSA-IPD at n_fft 1024 and 256, through the reference's own
dataset/salsa_lite_feature_extraction.py extract_features (which has no assert on n_fft) on one seeded 4-channel synth clip per case:
  * lite_nfft1024, ipd_nfft1024            n_fft 1024, hop 300 (F = 382 at the defaults);
  * lite_nfft1024_w800                     the same with win_len 800 in the YAML (the Lite script reads win_len and never uses it);
  * lite_nfft256, ipd_nfft256              n_fft 256, hop 150.
Per case: the clip's spatial channels every 4th frame and its log-spectrogram channels every 10th (the first and the last frame are
among both; the whole arrays would exceed the size limit of a committed file), the scaler's mean / std over ALL frames, the file names
of the feature tree, and in the meta the reference's lower_bin / upper_bin / cutoff_bin, F and T.
Writes only g26 (savez archives are not byte-reproducible: the other fixtures are not regenerated).  Build-container only (needs
the reference)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs ref_shims, imports the reference; its generators run only as a script)

N = 60000            # 2.5 s at 24 kHz: T = 201 (hop 300) / 401 (hop 150)
SPATIAL_STRIDE, LOGSPEC_STRIDE = 4, 10
CASES = [
    ('lite_nfft1024', dict(kind='salsa_lite', seed=2601, n_fft=1024, hop=300)),
    ('ipd_nfft1024', dict(kind='salsa_ipd', seed=2602, n_fft=1024, hop=300)),
    ('lite_nfft1024_w800', dict(kind='salsa_lite', seed=2603, n_fft=1024, hop=300, win=800)),
    ('lite_nfft256', dict(kind='salsa_lite', seed=2604, n_fft=256, hop=150)),
    ('ipd_nfft256', dict(kind='salsa_ipd', seed=2605, n_fft=256, hop=150)),
]


def main():
    meta, arrays = {'what': 'SALSA-Lite / IPD at n_fft 1024 and 256 through the reference', 'cases': {}}, {}
    for name, c in CASES:
        m, a = mg.ref_case(name, c['kind'], 'mic', {'fold1_room1_mix001': (c['seed'], N)}, n_fft=c['n_fft'], hop=c['hop'],
                           win=c.get('win'), fmax=2000, task='feature_scaler', stride=LOGSPEC_STRIDE)
        # the reference's statements (salsa_lite_feature_extraction.py:50-58) on this case's numbers
        fs, n_fft = m['fs'], m['n_fft']
        fmax = np.min((m['fmax_doa'], fs // 2))
        lower = int(np.max((1, int(np.floor(m['fmin_doa'] * n_fft / float(fs))))))
        upper = int(np.floor(fmax * n_fft / float(fs)))
        cutoff = int(np.floor(9000 * n_fft / float(fs)))
        spatial = a['%s|fold1_room1_mix001|spatial' % name]
        m.update(lower_bin=lower, upper_bin=upper, cutoff_bin=cutoff, F=int(spatial.shape[2]), T=int(spatial.shape[1]),
                 spatial_stride=SPATIAL_STRIDE)
        assert spatial.shape[2] == cutoff - lower and (m['T'] - 1) % SPATIAL_STRIDE == 0 and (m['T'] - 1) % LOGSPEC_STRIDE == 0
        a['%s|fold1_room1_mix001|spatial' % name] = spatial[:, ::SPATIAL_STRIDE].copy()
        meta['cases'][name] = m
        arrays.update(a)
        print(name, 'bins', lower, upper, cutoff, 'feature', (7,) + spatial.shape[1:], m['files'])
    mg.save('g26_lite_nfft', meta, **arrays)


if __name__ == '__main__':
    main()
