"""GPU tests of the scene renderer (salsa_amd/csrc/scene_render.hip) against the float64 restatement of its
definition in tests/scene_reference.py.  N = 4133 samples (nine blocks of 512, the last one short) at response lengths 1, 7, 512, 513,
1300 (one, two and three partitions, and a partition exactly full) and event lengths 1, 511, 512, 513, 3000, 4 and 6 channels (one and
two channel groups of the render kernel).  One batch per case holds the onsets 0, 1, 511, 512 and N - 1, an event that exactly fits, a
tail cut at N, three overlapping items with different responses and gains, and an empty clip.

Bound per case: max |out - ref64| <= 4 Y + ulp32(max |ref64|), Y the largest error of four float32 evaluations of the same inputs on
the CPU (one-shot fftconvolve, overlap-save at 256 / 512 / 1024): section 9j's convention -- another summation order and another FFT
factorisation may not cost more than four times what these cost."""
import numpy as np
import pytest
import torch

import scene_reference as sr

pytestmark = pytest.mark.gpu

N = 4133
GUARD = 67                                                                     # floats on either side of the output: odd, so `out` is 4-byte aligned only
SENTINEL = -12345.5


def _case(L, ln, C):
    from salsa_amd import scenes as sc
    rng = np.random.RandomState(1000 * L + ln + C)
    pool = sc.EventPool([rng.randn(ln).astype(np.float32) * 0.3 for _ in range(3)], [0, 1, 2])
    h = rng.randn(3, C, L) * 10.0 ** (-2.0 * np.arange(L) / max(L, 8))         # a 40-dB decay over the response
    bank = sc.RirBank(h.astype(np.float32), [10, -60, 120], [0, 20, -30], 'foa')
    full = ln + L - 1
    clips = [[],
             [(0, 0, 0, 1.0, 0)], [(1, 1, 1, 0.7, 0)], [(2, 2, 511, 1.3, 0)], [(0, 1, 512, 0.9, 0)], [(1, 2, N - 1, 1.0, 0)],
             [(2, 0, max(0, N - full), 0.8, 0)],                               # exactly fitting (or, longer than the clip, cut from onset 0)
             [(0, 2, max(0, N - max(1, full // 2)), 1.1, 0)],                  # the tail cut at N
             [(0, 0, 100, 1.0, 0), (1, 1, 100 + ln // 2 + 3, 0.5, 1), (2, 2, 700, 0.25, 2)]]
    return sc.Scenes.from_items(N, clips, pool, bank), pool, bank


def _render_guarded(scenes, pool, bank, ambient):
    from salsa_amd import scenes as sc
    B, C = scenes.n_clips, bank.n_channels
    flat = torch.full((B * C * N + 2 * GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out = flat[GUARD:GUARD + B * C * N].view(B, C, N)
    got = sc.render_scenes(scenes, pool, bank, ambient=ambient, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all()), 'a guard band was written'
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('C', [4, 6])
@pytest.mark.parametrize('ln', [1, 511, 512, 513, 3000])
@pytest.mark.parametrize('L', [1, 7, 512, 513, 1300])
def test_render_against_float64(L, ln, C, monkeypatch):
    from salsa_amd import scenes as sc
    scenes, pool, bank = _case(L, ln, C)
    B = scenes.n_clips
    inside = sr.support(scenes, pool, bank, N)
    assert not inside[0].any() and inside[1:].any(axis=1).all()
    amb_np = (0.05 * np.random.RandomState(L + ln).randn(B, C, N)).astype(np.float32)
    for ambient in (None, amb_np):
        ref = sr.render64(scenes, pool, bank, N, ambient)
        Y, errs = sr.float32_yardstick(scenes, pool, bank, N, ambient, ref)
        bound = 4.0 * Y + sr.ulp32(np.abs(ref).max())
        amb = None if ambient is None else torch.from_numpy(ambient).cuda()
        out = _render_guarded(scenes, pool, bank, amb)
        got = out.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print('L %4d len %4d C %d ambient %d: err %.3g, Y %.3g (one-shot, 256, 512, 1024: %s), err / Y %.2f'
              % (L, ln, C, ambient is not None, err, Y, ' '.join('%.3g' % e for e in errs), err / Y))
        assert err <= bound
        # exact properties
        base = np.zeros_like(got) if ambient is None else ambient
        assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32)), 'an empty scene is the ambient'
        outside = np.broadcast_to(~inside[:, None, :], got.shape)
        assert np.array_equal(got[outside].view(np.uint32), base[outside].view(np.uint32)), 'outside the supports the output is the ambient'
        again = _render_guarded(scenes, pool, bank, amb)
        assert torch.equal(_bits(out), _bits(again)), 'two runs give equal bits'
        alone = sc.render_scenes(scenes[8], pool, bank, ambient=None if amb is None else amb[8:9].contiguous())
        assert torch.equal(_bits(alone[0]), _bits(out[8])), 'a clip does not depend on its batch'
        # the torch.fft leg of SALSA_HIP_SCENE=0 meets the same bound and the same exact properties
        monkeypatch.setattr(sc, 'HIP_SCENE', False)
        leg = sc.render_scenes(scenes, pool, bank, ambient=amb).cpu().numpy()
        monkeypatch.setattr(sc, 'HIP_SCENE', True)
        leg_err = float(np.abs(leg.astype(np.float64) - ref).max())
        print('    torch.fft leg: err %.3g, err / Y %.2f' % (leg_err, leg_err / Y))
        assert leg_err <= bound
        assert np.array_equal(leg[outside].view(np.uint32), base[outside].view(np.uint32))


def test_clip_one_of_three_equals_the_clip_alone_and_out_may_be_the_ambient():
    from salsa_amd import scenes as sc
    pool = sc.synth_event_pool(4, 2, 5, min_s=0.05, max_s=0.2)
    bank = sc.make_rir_bank('foa', [(30, 10), (-100, -20), (170, 40)], 900, rt60=0.25, seed=1)
    scenes = sc.draw_scenes(3, pool, bank, 24000, 8, gap_s=(0.05, 0.3))
    assert min(np.diff(scenes.clip_start)) >= 2
    amb = 0.01 * torch.randn(3, 4, 24000, device='cuda', generator=torch.Generator('cuda').manual_seed(3))
    both = sc.render_scenes(scenes, pool, bank, ambient=amb)
    alone = sc.render_scenes(scenes[1], pool, bank, ambient=amb[1:2].contiguous())
    assert torch.equal(_bits(both[1]), _bits(alone[0]))
    ref = sr.render64(scenes, pool, bank, 24000, amb.cpu().numpy())
    Y, _ = sr.float32_yardstick(scenes, pool, bank, 24000, amb.cpu().numpy(), ref)
    assert np.abs(both.cpu().numpy() - ref).max() <= 4 * Y + sr.ulp32(np.abs(ref).max())
    buf = amb.clone()
    assert sc.render_scenes(scenes, pool, bank, ambient=buf, out=buf) is buf and torch.equal(_bits(buf), _bits(both))
    mic = sc.make_rir_bank('mic', [(30, 10), (-100, -20), (170, 40)], 900, rt60=0.25, seed=1)
    wet = sc.render_scenes(scenes, pool, mic)
    ref = sr.render64(scenes, pool, mic, 24000)
    Y, _ = sr.float32_yardstick(scenes, pool, mic, 24000, None, ref)
    assert np.abs(wet.cpu().numpy() - ref).max() <= 4 * Y + sr.ulp32(np.abs(ref).max())


def test_a_batch_without_any_item_is_the_ambient():
    """n_items = 0 is a path of its own in the launcher: no item spectra, no workspace"""
    from salsa_amd import scenes as sc
    pool = sc.EventPool([np.ones(5, np.float32)], [0])
    bank = sc.make_rir_bank('foa', [(0, 0)], 7)
    scenes = sc.Scenes.from_items(N, [[], []], pool, bank)
    amb = torch.randn(2, 4, N, device='cuda', generator=torch.Generator('cuda').manual_seed(9))
    assert torch.equal(_bits(_render_guarded(scenes, pool, bank, amb)), _bits(amb))
    assert not bool(_render_guarded(scenes, pool, bank, None).any())


def test_offsets_past_two_to_the_31():
    """one channel of 2^31 + 5000 samples (8.6 GB) with one item behind sample 2^31: block starts, onsets and output indices that do
    not fit 32 bits.  The item's neighbourhood against float64, everything else zero, checked on the device."""
    from salsa_amd import scenes as sc
    big = (1 << 31) + 5000
    free = torch.cuda.mem_get_info()[0]
    assert free > 10 * 2 ** 30, 'this test wants 10 GB of device memory'
    rng = np.random.RandomState(31)
    pool = sc.EventPool([rng.randn(600).astype(np.float32)], [0])
    bank = sc.RirBank(rng.randn(1, 1, 7).astype(np.float32), [0], [0], 'foa')
    onset = (1 << 31) + 100
    scenes = sc.Scenes.from_items(big, [[(0, 0, onset, 0.5, 0)]], pool, bank)
    out = sc.render_scenes(scenes, pool, bank)
    assert tuple(out.shape) == (1, 1, big)
    assert not bool(out[0, 0, :onset].any()) and not bool(out[0, 0, onset + 606:].any())
    local = sc.Scenes.from_items(4900, [[(0, 0, 100, 0.5, 0)]], pool, bank)   # the same item on a clip that starts at 2^31
    ref = sr.render64(local, pool, bank, 4900)
    Y, _ = sr.float32_yardstick(local, pool, bank, 4900, None, ref)
    got = out[0, 0, 1 << 31:(1 << 31) + 4900].cpu().numpy().astype(np.float64)
    assert np.abs(got).max() > 0.1 and np.abs(got - ref[0, 0]).max() <= 4 * Y + sr.ulp32(np.abs(ref).max())


@pytest.mark.parametrize('L', [1, 64, 700])
def test_an_anechoic_foa_item_puts_its_label_into_every_bin(oracle, L):
    """end to end: render, extract with SalsaExtractor, read the direction back.  1e-5 is the feature path's parity bar to the oracle,
    2.0e-6 the largest deviation the float32 partitioned evaluation of the renderer produced on the CPU at L in {1, 64, 700}, times 4 as
    above; the count of non-zero bins must reach 0.9 x the oracle's on the float64 render, against a vacuous pass."""
    from salsa_amd import scenes as sc
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import _ar1
    pool = sc.EventPool([(0.1 * _ar1(np.random.RandomState(3).randn(24000))).astype(np.float32)], [2])
    bank = sc.make_rir_bank('foa', [(70, -20), (-130, 40)], L)
    scenes = sc.Scenes.from_items(48000, [[(0, 1, 9000, 0.8, 0)]], pool, bank)
    audio = sc.render_scenes(scenes, pool, bank)
    feat = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device('cuda:0')).extract(audio)[0].cpu().numpy()
    ref_feat = oracle.extract_salsa(sr.render64(scenes, pool, bank, 48000)[0].astype(np.float32), audio_format='foa', fmax_doa=9000)
    nz, ref_nz = (feat[4:] != 0).any(axis=0), (ref_feat[4:] != 0).any(axis=0)
    x, y, z = sc._unit(-130, 40)
    dev = np.abs(feat[4:][:, nz] - np.array([y, z, x])[:, None]).max()
    print('L %d: %d non-zero bins (oracle on float64 render: %d), largest deviation %.3g' % (L, nz.sum(), ref_nz.sum(), dev))
    assert dev <= 1e-5 + 4 * 2.0e-6
    assert nz.sum() >= 0.9 * ref_nz.sum() and ref_nz.sum() > 10000


@pytest.mark.parametrize('fmt', ['classwise', 'trackwise'])
def test_add_scenes_feeds_the_bank_and_a_training_step(fmt):
    from salsa_amd import scenes as sc
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor
    NC, n_samples = 12, 8 * 24000
    pool = sc.synth_event_pool(NC, 2, 1, max_s=1.2)
    rbank = sc.make_rir_bank('foa', [(a, e) for a in range(-170, 180, 60) for e in (-30, 10)], 1200, rt60=0.3, seed=2)
    scenes = sc.draw_scenes(2, pool, rbank, n_samples, 4, max_polyphony=3, allow_same_class=(fmt == 'trackwise'), gap_s=(0.1, 0.8))
    ex = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device('cuda:0'))
    width = NC * (3 if fmt == 'trackwise' else 1)
    bank = GpuFeatureBank(ex, n_classes=width, label_format=fmt)
    amb = 1e-3 * torch.randn(2, 4, n_samples, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    audio = sc.add_scenes(bank, scenes, pool, rbank, ambient=amb)
    assert tuple(audio.shape) == (2, 4, n_samples) and bank.names == ['scene_0000', 'scene_0001'] and bank.clip_len == [640, 640]
    bank.fit_scaler()
    bank.finalize()
    assert len(bank) == 2
    for b in range(2):
        sed, doa = sc.scene_labels(scenes[b], 80, NC, fmt)
        assert sed.sum() > 0
        assert np.array_equal(bank.sed_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), sed.view(np.uint32))
        assert np.array_equal(bank.doa_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), doa.view(np.uint32))
    x, sed, doa, names = bank.batch([0, 1])
    assert tuple(x.shape) == (2, 7, 640, 200) and tuple(sed.shape) == (2, 80, width) and tuple(doa.shape) == (2, 80, 3 * width)
    assert np.array_equal(sed[1].cpu().numpy(), sc.scene_labels(scenes[1], 80, NC, fmt)[0])
    tr = Trainer('cuda', seed=3, **(dict(output_format='multi_accdoa', n_classes=NC) if fmt == 'trackwise' else {}))
    losses = tr.train_step(x, sed, doa)
    assert all(bool(torch.isfinite(v)) for v in losses)

