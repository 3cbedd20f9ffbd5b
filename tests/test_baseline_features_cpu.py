"""CPU checks of the baseline SELD features (dataset/feature_extraction.py): the float64 restatement reproduces the reference's
outputs (g21), the library's host mel matrix is librosa 0.8.0's, directory names / shapes / lag order / exceptions follow the
reference, the scaler math reproduces the reference's scaler files, and include/salsa_baseline.h matches its export list."""
import os
import re

import numpy as np
import pytest

import baseline_reference as br
from conftest import ROOT, golden_clip, load_golden


@pytest.fixture(scope='module')
def g21():
    return load_golden('g21_baseline')


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def case_clip(c):
    y = golden_clip(c['seed'], c['n'], c['sha'])
    if c['silence']:
        y = y.copy()
        y[:, c['silence'][0]:c['silence'][1]] = 0.0
    return y


def test_restatement_reproduces_g21(g21):
    meta, a = g21
    assert {c['feature_type'] for c in meta['cases']} == {'melspec', 'melspeciv', 'melspecgcc', 'linspeciv', 'linspecgcc'}
    for c in meta['cases']:
        ref = a[c['name']]
        out = br.extract(c['feature_type'], case_clip(c), c['fs'], c['n_fft'], c['hop'], c['win'], c['n_mels'], c['fmin'],
                         c['fmax'], c['compress'])
        assert out.shape == ref.shape, c['name']
        np.testing.assert_allclose(out[:4], ref[:4], rtol=1e-5, atol=2e-5, err_msg=c['name'])
        np.testing.assert_allclose(out[4:], ref[4:], rtol=1e-5, atol=1e-6, err_msg=c['name'])


def test_mel_matrix_is_librosas(g21, lib):
    from salsa_amd.baseline_features import mel_matrix
    _, a = g21
    assert np.array_equal(mel_matrix(24000, 512, 128, 50, 12000), a['melW_512_128'])
    assert np.array_equal(mel_matrix(24000, 256, 64, 50, 12000), a['melW_256_64'])
    for fs, n_fft, n_mels, fmin, fmax in ((16000, 512, 40, 0, 8000), (48000, 512, 96, 100, 20000), (24000, 256, 128, 50, 12000)):
        ours, ref = mel_matrix(fs, n_fft, n_mels, fmin, fmax), br.mel_matrix(fs, n_fft, n_mels, fmin, fmax)
        ulps = np.abs(ours.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert (ulps[(ours != 0) | (ref != 0)] <= 1).all()


def test_shapes_names_lags_and_exceptions(g21, lib):
    from salsa_amd import baseline_features as bf
    meta, a = g21
    for c in meta['cases']:
        assert bf.output_shape(c['feature_type'], c['n'], c['n_fft'], c['hop'], c['n_mels'], c['compress']) == a[c['name']].shape
    for t in meta['trees']:
        desc, _ = bf.feature_description(t['feature_type'], 24000, 512, 300, 128)
        assert all(k.split('|')[1] == desc for k in t['keys'])
    assert bf.feature_description('linspecgcc', 24000, 256, 150, 128) == ('24000fs_256nfft_150nhop_100nfreqs', 100)
    assert bf.feature_description('linspeciv', 24000, 512, 300, 128, False) == ('24000fs_512nfft_300nhop_256nfreqs', 256)
    assert bf.feature_description('melspecgcc', 24000, 512, 300, 64) == ('24000fs_512nfft_300nhop_64nmels', 64)
    # lag order: cc[-L//2:] ++ cc[:L//2], odd L included
    assert list(bf.gcc_lags(4, 16)) == [14, 15, 0, 1] and list(bf.gcc_lags(5, 16)) == [13, 14, 15, 0, 1]
    assert bf.PAIRS == tuple(br.PAIRS)
    with pytest.raises(AssertionError):
        bf.select_extractor('linspeciv', 24000, 1024, 300, 128)
    with pytest.raises(AssertionError):
        bf.feature_description('linspecgcc', 24000, 1024, 300, 128)
    with pytest.raises(NotImplementedError):
        bf.select_extractor('salsa', 24000, 512, 300, 128)
    with pytest.raises(NotImplementedError):
        bf.output_shape('spectrogram', 24000)
    with pytest.raises(AssertionError):
        bf.select_extractor('melspeciv', 24000, 512, 300, 128, win_length=1024)
    ex = bf.select_extractor('linspecgcc', 24000, 512, 300, 200)
    assert isinstance(ex, bf.LogSpecGccExtractor) and ex.n_freqs == 200 and ex.W.shape == (200, 257)
    assert bf.select_extractor('linspeciv', 24000, 512, 300, 256).n_freqs == 256
    mel = bf.select_extractor('melspecgcc', 24000, 512, 300, 128, fmin=50, fmax=12000)
    assert isinstance(mel, bf.MelSpecGccExtractor) and np.array_equal(mel.melW, a['melW_512_128'])


def test_scaler_math_reproduces_g21(g21):
    from salsa_amd.baseline_features import scaler_stats
    meta, a = g21
    for t in meta['trees']:
        pre = 'tree_%s|%s|' % (t['format'], t['feature_type'])
        feats = [a[k] for k in sorted(a) if k.startswith(pre) and '_dev|' in k and k.endswith('|feature')]
        assert len(feats) == 2
        got = scaler_stats(feats)
        for name, g in zip(('mean', 'std', 'scalar_mean', 'scalar_std'), got):
            ref = a[[k for k in a if k.startswith(pre) and k.endswith('_feature_scaler.h5|' + name)][0]]
            assert g.shape == ref.shape and g.dtype == np.float32, name
            np.testing.assert_allclose(g, ref, rtol=2e-6, atol=1e-6, err_msg=name)


def test_header_symbols_are_the_export_list(lib):
    from salsa_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'salsa_baseline.h')).read(), flags=re.S)
    names = set(re.findall(r'\b(salsa_baseline_[a-z_]+)\s*\(', hdr))
    assert names == set(_lib.BASELINE_EXPORTS) and len(names) == 6
    assert all(hasattr(lib, n) for n in names)
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'baseline_kernels.hip') in _lib.build_command()
    import ctypes as C
    assert C.sizeof(_lib.BaselineParams) == 48


def test_library_refuses_bad_plans_on_the_host(lib):
    """checks that run before any device call of salsa_baseline_plan_create"""
    import ctypes as C
    from salsa_amd import _lib
    p = _lib.BaselineParams(fs=24000, n_fft=1024, hop_len=300, win_len=1024, n_mels=128, feature_type=1, fmin=50, fmax=12000,
                            is_compressed_freq=1, reserved=0)
    plan = C.c_void_p()
    assert lib.salsa_baseline_plan_create(C.byref(p), C.byref(plan)) == _lib.E_NFFT and not plan.value
    p.n_fft, p.win_len = 512, 600
    assert lib.salsa_baseline_plan_create(C.byref(p), C.byref(plan)) == _lib.E_INVAL
    assert b'Windown length' in lib.salsa_last_error()
    p.win_len, p.feature_type = 512, 7
    assert lib.salsa_baseline_plan_create(C.byref(p), C.byref(plan)) == _lib.E_INVAL
    p.feature_type, p.n_mels = 2, 2048
    assert lib.salsa_baseline_plan_create(C.byref(p), C.byref(plan)) == _lib.E_INVAL
