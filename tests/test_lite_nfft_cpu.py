"""SALSA-Lite / SALSA-IPD at n_fft 1024 (and the n_fft 256 cases no fixture held), host side: the CPU oracle against the reference's
own output (fixture g26, tools/make_golden_lite_nfft.py), the host arithmetic of the sizes, and the checks salsa_plan_create makes
before it touches a device.  Tolerances as tests/test_oracle_golden.py: float64-accurate values, indices and the zeroed band exact."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_clip, load_golden
from golden_cases import lite_period

CASES = ['lite_nfft1024', 'ipd_nfft1024', 'lite_nfft1024_w800', 'lite_nfft256', 'ipd_nfft256']
CLIP = 'fold1_room1_mix001'


def _case(name):
    meta, a = load_golden('g26_lite_nfft')
    c = meta['cases'][name]
    seed, n, fs, sha = c['clips'][CLIP]
    assert fs == 24000
    return c, golden_clip(seed, n, sha), a['%s|%s|spatial' % (name, CLIP)], a['%s|%s|logspec' % (name, CLIP)], a[name + '|mean'], a[name + '|std']


@pytest.mark.parametrize('name', CASES)
def test_oracle_lite_matches_reference_golden(oracle, name):
    c, y, spatial, logspec, mean, std = _case(name)
    out = oracle.extract_lite(y, fs=c['fs'], n_fft=c['n_fft'], hop=c['hop'], win=c['win'], fmin_doa=c['fmin_doa'], fmax_doa=c['fmax_doa'],
                              feature_type=c['kind'])
    assert out.shape == (7, c['T'], c['F']) and out.dtype == np.float32
    assert oracle.bin_limits(c['fs'], c['n_fft'], c['fmin_doa'], c['fmax_doa']) == (c['lower_bin'], c['upper_bin'], c['cutoff_bin'])
    got_sp, got_ls = out[4:, ::c['spatial_stride']], out[:4, ::c['stride']]
    assert got_sp.shape == spatial.shape and got_ls.shape == logspec.shape
    # lite :120 zeroes the phase rows from index upper_bin of the CROPPED axis on: exactly zero on both sides, nothing else zeroed wholesale
    up = c['upper_bin']
    assert not spatial[:, :, up:].any() and not got_sp[:, :, up:].any()
    assert np.array_equal(got_sp == 0, spatial == 0)
    # float64-accurate values rounded to float32 on both sides: one float32 rounding apart at most; phases modulo one turn in the
    # mirror-symmetric frame 0 (real spectra up to round-off: the sign of a +-pi phase is decided by that round-off in the reference too)
    np.testing.assert_allclose(got_ls, logspec, rtol=2e-6, atol=2e-5)
    d = got_sp.astype(np.float64) - spatial
    wraps = np.round(d / lite_period(c, c['lower_bin'], c['F']))
    d -= wraps * lite_period(c, c['lower_bin'], c['F'])
    assert np.abs(d).max() <= 1e-6
    assert set(np.unique(np.nonzero(wraps)[1])) <= {0}
    m, s = oracle.compute_scaler([out])
    np.testing.assert_allclose(m, mean, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(s, std, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('name', CASES)
def test_host_sizes_equal_the_golden_meta(name):
    """salsa_bin_limits and the host-side output shape (what torch.ops.salsa.extract's fake implementation returns)"""
    from salsa_amd.extractor import bin_limits
    from salsa_amd.torch_ops import output_shape
    c = _case(name)[0]
    assert bin_limits(c['fs'], c['n_fft'], c['fmin_doa'], c['fmax_doa']) == (c['lower_bin'], c['upper_bin'], c['cutoff_bin'])
    n = c['clips'][CLIP][1]
    assert output_shape(n, 'mic', c['kind'], c['fs'], c['n_fft'], c['hop'], c['fmin_doa'], c['fmax_doa']) == (7, c['T'], c['F'])


def test_default_sizes_at_1024():
    c = _case('lite_nfft1024')[0]
    assert (c['lower_bin'], c['upper_bin'], c['cutoff_bin'], c['F']) == (2, 85, 384, 382)


def test_host_shape_refuses_what_the_plan_refuses():
    from salsa_amd.torch_ops import output_shape
    for kw in (dict(feature_type='salsa', n_fft=1024), dict(feature_type='salsa_lite', n_fft=128), dict(feature_type='salsa_lite', n_fft=2048),
               dict(feature_type='salsa_ipd', n_fft=1000)):
        with pytest.raises(AssertionError):
            output_shape(24000, 'mic', **kw)


def test_plan_create_checks_before_any_device_call():
    """n_fft is checked first, then the format (the order salsa_plan_create applies at 512); none of these reaches a device"""
    from salsa_amd import _lib
    lib = _lib.load()

    def create(**kw):
        d = dict(fs=24000, n_fft=512, hop_len=300, win_len=kw.get('n_fft', 512), fmin_doa=50, fmax_doa=2000, cond_num=5.0, n_hopframes=3,
                 is_tracking=1, is_compress_high_freq=1, audio_format=_lib.FORMAT['mic'], feature_type=_lib.FEATURE['salsa_lite'],
                 audio_layout=0, flags=0, floor_mask_ratio=0.0, fmax_spec=0, reserved=0)
        d.update(kw)
        p, plan = _lib.SalsaParams(**d), C.c_void_p()
        rc = lib.salsa_plan_create(C.byref(p), C.byref(plan))
        assert rc != 0 and not plan.value
        return rc

    for ft in ('salsa_lite', 'salsa_ipd'):
        for n_fft in (128, 1000, 2048):
            assert create(n_fft=n_fft, feature_type=_lib.FEATURE[ft]) == _lib.E_NFFT
    for fmt in ('foa', 'mic'):
        assert create(n_fft=1024, feature_type=_lib.FEATURE['salsa'], audio_format=_lib.FORMAT[fmt]) == _lib.E_NFFT
    assert create(n_fft=1024, flags=_lib.FLAG_FLEX) == _lib.E_NFFT                      # the contrib surface stays at 256 / 512
    for n_fft in (512, 1024):                                                           # Lite is MIC only: the same refusal at both sizes
        assert create(n_fft=n_fft, audio_format=_lib.FORMAT['foa']) == _lib.E_FORMAT
        assert 'only for MIC' in _lib.last_error()
    assert create(n_fft=1024, audio_format=7) == _lib.E_FORMAT
    assert create(n_fft=1024, fmax_doa=9500) == _lib.E_BINS                             # lite :59, before any device call as well
