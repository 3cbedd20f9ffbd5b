"""SALSA-Lite / SALSA-IPD at n_fft 1024 on the device (stft_kernel<1024, ...>: two 512-point half transforms joined in registers), and
the n_fft 256 cases no fixture held: against the reference's own output (fixture g26) and against the CPU oracle at full size.
Bars as tests/test_gpu_parity.py: shapes, indices and the zeroed band exact, floats within 1e-5 relative (2e-5 dB / 1e-6 absolute)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_clip, load_golden
from golden_cases import lite_period
from salsa_amd.synth import synth_clip

pytestmark = pytest.mark.gpu

RTOL, ATOL_DB, ATOL_SP = 1e-5, 2e-5, 1e-6
CASES = ['lite_nfft1024', 'ipd_nfft1024', 'lite_nfft1024_w800', 'lite_nfft256', 'ipd_nfft256']
CLIP = 'fold1_room1_mix001'


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _extractor(**kw):
    from salsa_amd.extractor import SalsaExtractor
    return SalsaExtractor(audio_format='mic', **kw)


def _case_kwargs(c):
    return dict(feature_type=c['kind'], fs=c['fs'], n_fft=c['n_fft'], hop_len=c['hop'], win_len=c['win'], fmin_doa=c['fmin_doa'],
                fmax_doa=c['fmax_doa'])


def _check(out_ls, out_sp, ref_ls, ref_sp, c, what, mirror=(0,)):
    """log-spectrogram planes and phase planes against a reference, each on its own frame subset.  The phase of a mirror-symmetric
    frame (frame 0 here: real spectra up to round-off) may differ by one whole turn where it is +-pi, as in tests/test_gpu_parity.py."""
    assert out_ls.shape == ref_ls.shape and out_sp.shape == ref_sp.shape and out_ls.dtype == out_sp.dtype == np.float32
    up = c['upper_bin']
    assert not out_sp[:, :, up:].any() and not ref_sp[:, :, up:].any()             # lite :120, on the cropped axis
    plain = np.setdiff1d(np.arange(out_sp.shape[1]), list(mirror))                  # (a mirror-symmetric frame's phases are round-off of 0 or
    assert np.array_equal(out_sp[:, plain] == 0, ref_sp[:, plain] == 0)             # pi on both sides: whether one is exactly 0 is not pinned)
    e_ls = np.abs(out_ls.astype(np.float64) - ref_ls)
    bound_ls = ATOL_DB + RTOL * np.abs(ref_ls)
    period = lite_period(c, c['lower_bin'], c['F'])
    d = out_sp.astype(np.float64) - ref_sp
    wraps = np.round(d / period)
    d = np.abs(d - period * wraps)
    bound_sp = ATOL_SP + RTOL * np.abs(ref_sp)
    print('%s: log-spectrogram max err %.3g (bound %.3g, worst ratio %.3f); phase max err %.3g (bound >= %.3g, worst ratio %.3f); wrapped frames %s'
          % (what, e_ls.max(), ATOL_DB, (e_ls / bound_ls).max(), d.max(), ATOL_SP, (d / bound_sp).max(), sorted(set(np.nonzero(wraps)[1]))))
    assert np.all(e_ls <= bound_ls)
    assert np.all(d <= bound_sp)
    assert set(np.nonzero(wraps)[1]) <= set(mirror)


def _golden(name):
    meta, a = load_golden('g26_lite_nfft')
    c = meta['cases'][name]
    seed, n, fs, sha = c['clips'][CLIP]
    return c, golden_clip(seed, n, sha), a


@pytest.mark.parametrize('name', CASES)
def test_extract_matches_reference_golden(dev, name):
    c, y, a = _golden(name)
    ex = _extractor(**_case_kwargs(c))
    assert ex.output_shape(y.shape[1]) == (7, c['T'], c['F'])
    out = ex.extract(torch.from_numpy(y[None]).to(dev))[0].cpu().numpy()
    assert out.shape == (7, c['T'], c['F'])
    _check(out[:4, ::c['stride']], out[4:, ::c['spatial_stride']], a['%s|%s|logspec' % (name, CLIP)], a['%s|%s|spatial' % (name, CLIP)], c, name)


@pytest.mark.parametrize('ftype', ['salsa_lite', 'salsa_ipd'])
def test_60s_clip_and_batch_of_32_against_oracle(dev, oracle, ftype):
    """the benchmark's shape at n_fft 1024: 32 clips of 60 s.  Clips 0, 13 and 31 against the oracle in full, every clip by determinism,
    batch-order invariance, the zeroed band and finiteness; clip 0 alone (a batch of one) equals its row of the batch bit for bit."""
    B, n = 32, 60 * 24000
    ys = np.stack([synth_clip(2600 + i, n) for i in range(B)])
    ex = _extractor(feature_type=ftype, n_fft=1024, fmax_doa=2000)
    a = torch.from_numpy(ys).to(dev)
    out1 = ex.extract(a)
    out2 = ex.extract(a)
    assert torch.equal(out1, out2)
    assert tuple(out1.shape) == (B, 7, 4801, 382)
    assert torch.isfinite(out1).all() and not out1[:, 4:, :, 85:].any()
    assert torch.equal(torch.flip(ex.extract(torch.flip(a, dims=[0]).contiguous()), dims=[0]), out1)
    assert torch.equal(ex.extract(a[:1].contiguous())[0], out1[0])
    c = dict(kind=ftype, fs=24000, n_fft=1024, lower_bin=2, upper_bin=85, F=382)
    assert oracle.bin_limits(24000, 1024, 50, 2000) == (2, 85, 384)
    for i in (0, 13, 31):
        ref = oracle.extract_lite(ys[i], n_fft=1024, fmax_doa=2000, feature_type=ftype)
        o = out1[i].cpu().numpy()
        _check(o[:4], o[4:], ref[:4], ref[4:], c, '%s 60 s clip %d' % (ftype, i))


def test_interleaved_layout_and_scaler_at_1024(dev):
    """interleaved audio gives the planar result bit for bit; an attached scaler (read from global memory at F = 382) equals the separate
    normalisation of the raw output within one rounding of the division"""
    from salsa_amd.extractor import normalize_
    ys = np.stack([synth_clip(2650 + i, 3 * 24000) for i in range(3)])
    a = torch.from_numpy(ys).to(dev)
    for ftype in ('salsa_lite', 'salsa_ipd'):
        planar = _extractor(feature_type=ftype, n_fft=1024, fmax_doa=2000)
        raw = planar.extract(a).clone()
        inter = _extractor(feature_type=ftype, n_fft=1024, fmax_doa=2000, audio_layout='interleaved')
        assert torch.equal(inter.extract(a.permute(0, 2, 1).contiguous()), raw)
        g = torch.Generator().manual_seed(26)
        mean, std = torch.randn(4, 382, generator=g) * 10 - 40, torch.rand(4, 382, generator=g) * 10 + 5
        planar.set_scaler(mean, std)
        fused = planar.extract(a)
        sep = normalize_(raw.clone(), mean.to(dev), std.to(dev))
        assert torch.equal(fused[:, 4:], raw[:, 4:])
        torch.testing.assert_close(fused[:, :4], sep[:, :4], rtol=1e-6, atol=1e-6)


def _tree(tmp, clips, c, int16=False):
    import yaml
    from scipy.io import wavfile
    data_dir, feat_dir = os.path.join(tmp, 'data'), os.path.join(tmp, 'feat')
    os.makedirs(os.path.join(data_dir, 'mic_dev'), exist_ok=True)
    os.makedirs(os.path.join(data_dir, 'mic_eval'), exist_ok=True)
    for name, y in clips.items():
        if int16:
            y = np.clip(y / np.abs(y).max() * 30000, -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(data_dir, 'mic_dev', name + '.wav'), 24000, y.T)       # float32 WAV: samples survive exactly
    cfg = {'data_dir': data_dir, 'feature_dir': feat_dir,
           'data': {'format': 'mic', 'fs': c['fs'], 'n_fft': c['n_fft'], 'win_len': c['win'], 'hop_len': c['hop'], 'fmin_doa': c['fmin_doa'],
                    'fmax_doa': c['fmax_doa']}}
    path = os.path.join(tmp, 'cfg.yml')
    with open(path, 'w') as f:
        yaml.safe_dump(cfg, f)
    return path, feat_dir


@pytest.mark.parametrize('name', ['lite_nfft1024', 'ipd_nfft1024', 'lite_nfft1024_w800'])
def test_lite_harness_reproduces_reference_tree(dev, tmp_path, name):
    """lite_features.extract_features with n_fft: 1024 in the YAML: the reference's directory and file names, feature file and scaler"""
    from salsa_amd import io as sio
    from salsa_amd import lite_features
    c, y, a = _golden(name)
    cfg, feat_dir = _tree(str(tmp_path), {CLIP: y}, c)
    lite_features.extract_features(data_config=cfg, feature_type=c['kind'], batch_size=2)
    assert '24000fs_1024nfft_300nhop_2000fmaxdoa' in c['files'][CLIP]
    got = sio.load_arrays(os.path.join(feat_dir, *c['files'][CLIP].split('|')))['feature']
    assert got.shape == (7, c['T'], c['F']) and got.dtype == np.float32
    _check(got[:4, ::c['stride']], got[4:, ::c['spatial_stride']], a['%s|%s|logspec' % (name, CLIP)], a['%s|%s|spatial' % (name, CLIP)], c, name)
    sc = sio.load_arrays(os.path.join(feat_dir, *c['files']['scaler'].split('|')))
    np.testing.assert_allclose(sc['mean'], a[name + '|mean'], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(sc['std'], a[name + '|std'], rtol=1e-5, atol=1e-5)


def test_raw_pcm_upload_equals_host_decoding_at_1024(dev, tmp_path):
    """16-bit WAV clips: the pipeline that uploads the file's bytes and converts on the device writes the same feature files, bit for
    bit, as the pipeline that decodes on the host and uploads planar float32"""
    from salsa_amd import features, io as sio
    from salsa_amd import lite_features
    c = _golden('lite_nfft1024')[0]
    clips = {'c%d' % i: synth_clip(2680 + i, n) for i, n in enumerate([48000, 48000, 36001, 47700])}
    trees = {}
    for raw in (True, False):
        d = tmp_path / ('raw%d' % raw)
        d.mkdir()
        cfg, feat_dir = _tree(str(d), clips, c, int16=True)
        features.RAW_PCM = raw
        try:
            lite_features.extract_features(data_config=cfg, feature_type='salsa_lite', task='feature', batch_size=2)
        finally:
            features.RAW_PCM = True
        root = os.path.join(feat_dir, 'salsa_lite', 'mic', '24000fs_1024nfft_300nhop_2000fmaxdoa', 'mic_dev')
        trees[raw] = {fn: sio.load_arrays(os.path.join(root, fn))['feature'] for fn in sio.feature_files(root)}
    assert sorted(trees[True]) == sorted(trees[False]) and len(trees[True]) == 4
    for fn in trees[True]:
        assert trees[True][fn].shape[2] == 382 and np.array_equal(trees[True][fn], trees[False][fn]), fn


def test_refusals_that_remain(dev):
    with pytest.raises(AssertionError):
        _extractor(feature_type='salsa', n_fft=1024)
    for n_fft in (128, 1000, 2048):
        with pytest.raises(AssertionError):
            _extractor(feature_type='salsa_lite', n_fft=n_fft)
    with pytest.raises(AssertionError):
        from salsa_amd.extractor import SalsaExtractor
        SalsaExtractor(audio_format='foa', feature_type='salsa_lite', n_fft=1024)
    ex = _extractor(feature_type='salsa_lite', n_fft=1024, fmax_doa=2000)
    with pytest.raises(AssertionError):
        ex.logspec(torch.zeros(1, 4, 24000, device=dev))                               # MagStftExtractor's sizes are 256 / 512
