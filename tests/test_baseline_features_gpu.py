"""GPU tests of the baseline SELD features (salsa_amd/baseline_features.py -> baseline_kernels.hip): the reference's outputs (g21),
the float64 restatement at 32 x 60 s, the lin types' log rows against SalsaExtractor.logspec, GCC peaks at known delays,
digital silence, the extract_features tree with its scaler file, and hipGraph capture."""
import os

import numpy as np
import pytest
import yaml

import baseline_reference as br
from conftest import load_golden
from test_baseline_features_cpu import case_clip

pytestmark = pytest.mark.gpu
ATOL_DB, RTOL = 2e-5, 1e-5


@pytest.fixture(scope='module')
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ex(ft, **kw):
    from salsa_amd.baseline_features import BaselineExtractor
    return BaselineExtractor(feature_type=ft, **kw)


def _check(out, ref, ft, name='', iv_outliers=0.0):
    """iv_outliers: the fraction of IV values allowed outside atol 1e-6 + rtol 1e-5 (then within 1e-4).  IV / ||IV|| is a ratio of
    near-cancelling products in a few bins per million, where one float32 ulp of the STFT (float64 FFTs in another order) moves
    it by more than the tolerance; g21 holds every value to the tolerance, 32 x 60 s of audio holds all but those."""
    assert out.shape == ref.shape, name
    np.testing.assert_allclose(out[:4], ref[:4], rtol=RTOL, atol=ATOL_DB, err_msg=name)
    if ft.endswith('iv'):
        bad = np.abs(out[4:] - ref[4:]) > 1e-6 + 1e-5 * np.abs(ref[4:])
        if iv_outliers and bad.mean() <= iv_outliers:
            np.testing.assert_allclose(out[4:], ref[4:], rtol=0, atol=1e-4, err_msg=name)
        else:
            np.testing.assert_allclose(out[4:], ref[4:], rtol=1e-5, atol=1e-6, err_msg=name)
    elif ft.endswith('gcc'):
        np.testing.assert_allclose(out[4:], ref[4:], rtol=0, atol=1e-5, err_msg=name)


def test_every_g21_case_matches_the_reference(dev):
    from salsa_amd.baseline_features import select_extractor
    meta, a = load_golden('g21_baseline')
    for c in meta['cases']:
        ex = select_extractor(c['feature_type'], c['fs'], c['n_fft'], c['hop'], c['n_mels'], c['win'], c['fmin'], c['fmax'])
        out = ex.extract(case_clip(c))
        assert out.dtype == np.float32
        _check(out, a[c['name']], c['feature_type'], c['name'])


def test_batch32_60s_matches_the_float64_restatement(dev):
    import torch
    from salsa_amd.synth import synth_clip, synth_clips_device
    audio = synth_clips_device(900, 32, device=dev)
    audio[5] = torch.from_numpy(synth_clip(77, 60 * 24000)).to(dev)
    for ft in ('melspec', 'melspeciv', 'melspecgcc', 'linspeciv', 'linspecgcc'):
        ex = _ex(ft, n_mels=128, fmin=50, fmax=12000)
        out = ex.extract(audio)
        assert tuple(out.shape) == (32,) + ex.output_shape(60 * 24000)
        for i in (5, 31):
            ref = br.extract(ft, audio[i].cpu().numpy(), n_mels=128, fmin=50, fmax=12000)
            _check(out[i].cpu().numpy(), ref, ft, '%s clip %d' % (ft, i), iv_outliers=1e-5)
        del out


def test_lin_log_rows_equal_salsa_logspec(dev):
    import torch
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import synth_clip
    a = torch.from_numpy(np.stack([synth_clip(31 + i, 24000) for i in range(3)])).to(dev)
    for n_fft, hop, comp in ((512, 300, True), (256, 150, True), (512, 240, False)):
        ref = SalsaExtractor(n_fft=n_fft, hop_len=hop, is_compress_high_freq=comp, device=dev).logspec(a).cpu().numpy()
        for ft in ('linspeciv', 'linspecgcc'):
            out = _ex(ft, n_fft=n_fft, hop_len=hop, is_compressed_freq=comp).extract(a).cpu().numpy()
            np.testing.assert_allclose(out[:, :4], ref, rtol=RTOL, atol=ATOL_DB)


def test_gcc_peak_sits_at_the_known_delay(dev):
    import torch
    rng = np.random.RandomState(5)
    src = rng.randn(24000).astype(np.float32)
    delays = (0, 3, 7, 12)                                   # channel c = source delayed by delays[c] samples
    y = np.stack([np.roll(src, d) for d in delays]).astype(np.float32)
    from salsa_amd.baseline_features import PAIRS
    for ft, F in (('linspecgcc', 200), ('melspecgcc', 128)):
        out = _ex(ft, n_mels=128, fmin=50, fmax=12000).extract(torch.from_numpy(y[None]).to(dev))[0].cpu().numpy()
        mid = out[4:, 5:-5].mean(axis=1)                     # frames away from the clip ends (reflect padding)
        for p, (n, m) in enumerate(PAIRS):
            # R = X_m conj(X_n): cc peaks at lag d_m - d_n, stored at index F//2 + lag
            assert int(np.argmax(mid[p])) == F // 2 + delays[m] - delays[n], (ft, n, m)
            assert mid[p].max() > 0.5


def test_digital_silence(dev):
    import torch
    y = torch.zeros((2, 4, 12000), dtype=torch.float32, device=dev)
    iv = _ex('linspeciv').extract(y).cpu().numpy()
    assert (iv[:, 4:] == 0).all() and np.allclose(iv[:, :4], -100.0)
    for ft, F in (('linspecgcc', 200), ('melspecgcc', 128)):
        g = _ex(ft, n_mels=128, fmin=50, fmax=12000).extract(y).cpu().numpy()[:, 4:]
        delta = np.zeros(F, np.float32)
        delta[F // 2] = 1.0
        np.testing.assert_allclose(g, np.broadcast_to(delta, g.shape), atol=1e-6)


def test_extract_features_writes_the_reference_tree(dev, tmp_path):
    from scipy.io import wavfile
    from salsa_amd import io as sio
    from salsa_amd.baseline_features import extract_features
    meta, a = load_golden('g21_baseline')
    from conftest import golden_clip
    for t in meta['trees']:
        root = tmp_path / t['format']
        data_dir, feat_dir = root / 'data', root / 'feat'
        fmt = t['format']
        for i, (seed, n, sha) in enumerate(zip(t['seeds'], t['lengths'], t['shas'])):
            split = fmt + ('_dev' if i < 2 else '_eval')
            os.makedirs(data_dir / split, exist_ok=True)
            name = 'fold%d_room1_mix%03d.wav' % (1 if i < 2 else 2, seed - 2139)
            wavfile.write(str(data_dir / split / name), 24000, golden_clip(seed, n, sha).T.copy())
        cfg = {'data_dir': str(data_dir), 'feature_dir': str(feat_dir),
               'data': {'format': fmt, 'fs': 24000, 'n_fft': 512, 'win_len': 512, 'hop_len': 300, 'fmin': 50, 'fmax': 12000,
                        'n_mels': 128}}
        cfg_path = root / 'cfg.yml'
        cfg_path.write_text(yaml.safe_dump(cfg))
        extract_features(str(cfg_path), feature_type=t['feature_type'], task='feature_scaler')
        for k in t['keys']:
            rel, dset = k.rsplit('|', 1)
            path = os.path.join(str(feat_dir), *rel.split('|'))
            got = sio.load_arrays(path)[dset]
            ref = a['tree_%s|%s' % (fmt, k)]
            assert got.dtype == np.float32 and got.shape == ref.shape, k
            if dset == 'feature':
                _check(got, ref, t['feature_type'], k)
            else:
                np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5, err_msg=k)
        scaler = os.path.join(str(feat_dir), t['feature_type'], rel.split('|')[1], fmt + '_feature_scaler.h5')
        assert set(sio.load_arrays(scaler if os.path.exists(scaler) else sio._alt(scaler))) == {'mean', 'std', 'scalar_mean', 'scalar_std'}


def test_extract_captures_and_replays_in_a_graph(dev):
    import torch
    from salsa_amd.synth import synth_clip
    a = torch.from_numpy(np.stack([synth_clip(60 + i, 30000) for i in range(2)])).to(dev)
    for ft in ('melspeciv', 'linspecgcc'):
        ex = _ex(ft, n_mels=128, fmin=50, fmax=12000)
        eager = ex.extract(a).clone()
        out = torch.empty_like(eager)
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            ex.extract(a, out=out)                            # warm-up on the side stream
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        out.zero_()
        with torch.cuda.graph(g):
            ex.extract(a, out=out)
        g.replay()
        torch.cuda.synchronize(dev)
        assert torch.equal(out, eager), ft


def test_short_clip_is_refused(dev):
    import torch
    with pytest.raises(ValueError):
        _ex('linspecgcc').extract(torch.zeros((1, 4, 512), dtype=torch.float32, device=dev))
    assert _ex('linspeciv').extract(torch.zeros((1, 4, 512), dtype=torch.float32, device=dev)).shape == (1, 7, 2, 200)
