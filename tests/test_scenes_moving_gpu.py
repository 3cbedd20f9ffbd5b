"""GPU tests of moving sources in the scene renderer (salsa_scene_render_moving) against the float64 restatement
in tests/scene_moving_reference.py.  N = 4133 samples; trajectory steps S of 240, 512, 700 and 2400 samples; event lengths 1, 2, S,
S + 1, 2 S + 1 and 3000 (one node, two nodes one sample apart, a last node exactly on and one sample past the event's end, and
segments longer and shorter than a partition); response lengths 1, 513 and 1300; 4 and 6 channels.  One batch per case holds an empty
clip, moving items at the onsets 0, 511, 512 and N - 1, a tail cut at N, a moving and a static item overlapping, two moving items
overlapping with different gains, and a trajectory that names one response throughout.

Bound per case, as in tests/test_scenes_gpu.py: max |out - ref64| <= 4 Y + ulp32(max |ref64|), Y the largest error of four float32
evaluations of the same inputs on the CPU, window included."""
import numpy as np
import pytest
import torch

import scene_moving_reference as mr
import scene_reference as sr

pytestmark = pytest.mark.gpu

N = 4133
GUARD = 67                                                                     # floats on either side of the output: odd, so `out` is 4-byte aligned only
SENTINEL = -12345.5


def _traj(ln, S, first, stride=1, R=4):
    from salsa_amd import scenes as sc
    return [(first + stride * k) % R for k in range(int(sc.traj_nodes(ln, S)))]


def _case(S, L, ln, C):
    from salsa_amd import scenes as sc
    rng = np.random.RandomState(100000 * (S % 97) + 1000 * L + ln + C)
    pool = sc.EventPool([rng.randn(ln).astype(np.float32) * 0.3 for _ in range(3)], [0, 1, 2])
    h = rng.randn(4, C, L) * 10.0 ** (-2.0 * np.arange(L) / max(L, 8))         # a 40-dB decay over the response
    bank = sc.RirBank(h.astype(np.float32), [10, -60, 120, -170], [0, 20, -30, 45], 'foa')
    full = ln + L - 1
    clips = [[],
             [(0, _traj(ln, S, 0), 0, 1.0, 0)], [(1, _traj(ln, S, 1), 511, 0.7, 0)], [(2, _traj(ln, S, 2, 3), 512, 1.3, 0)],
             [(1, _traj(ln, S, 3), N - 1, 1.0, 0)],
             [(0, _traj(ln, S, 2), max(0, N - max(1, full // 2)), 1.1, 0)],    # the tail cut at N
             [(0, _traj(ln, S, 0), 100, 1.0, 0), (1, 2, 100 + ln // 2 + 3, 0.5, 1)],                    # a moving and a static item overlapping
             [(1, _traj(ln, S, 1), 300, 0.8, 0), (2, _traj(ln, S, 0, 3), 300 + ln // 3 + 1, 0.3, 1)],  # two moving items, different gains
             [(2, [1] * len(_traj(ln, S, 0)), 700, 1.1, 0)]]                   # a trajectory that names one response throughout
    return sc.Scenes.from_items(N, clips, pool, bank, traj_step=S), pool, bank


def _render_guarded(scenes, pool, bank, ambient, **kw):
    from salsa_amd import scenes as sc
    B, C = scenes.n_clips, bank.n_channels
    flat = torch.full((B * C * N + 2 * GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    out = flat[GUARD:GUARD + B * C * N].view(B, C, N)
    got = sc.render_scenes(scenes, pool, bank, ambient=ambient, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[-GUARD:] == SENTINEL).all()), 'a guard band was written'
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lengths(S):
    return sorted({1, 2, S, S + 1, 2 * S + 1, 3000})


@pytest.mark.parametrize('C', [4, 6])
@pytest.mark.parametrize('L', [1, 513, 1300])
@pytest.mark.parametrize('S,ln', [(S, ln) for S in (240, 512, 700, 2400) for ln in _lengths(S)])
def test_moving_render_against_float64(S, ln, L, C, monkeypatch):
    from salsa_amd import scenes as sc
    scenes, pool, bank = _case(S, L, ln, C)
    B = scenes.n_clips
    inside = mr.support(scenes, pool, bank, N)
    assert not inside[0].any() and inside[1:].any(axis=1).all()
    amb_np = (0.05 * np.random.RandomState(L + ln).randn(B, C, N)).astype(np.float32)
    for ambient in (None, amb_np):
        ref = mr.render64_moving(scenes, pool, bank, N, ambient)
        Y, errs = mr.float32_yardstick(scenes, pool, bank, N, ambient, ref)
        bound = 4.0 * Y + sr.ulp32(np.abs(ref).max())
        amb = None if ambient is None else torch.from_numpy(ambient).cuda()
        out = _render_guarded(scenes, pool, bank, amb)
        got = out.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print('S %4d L %4d len %4d C %d ambient %d: err %.3g, Y %.3g (one-shot, 256, 512, 1024: %s), err / Y %.2f'
              % (S, L, ln, C, ambient is not None, err, Y, ' '.join('%.3g' % e for e in errs), err / Y))
        assert err <= bound
        # exact properties
        base = np.zeros_like(got) if ambient is None else ambient
        assert np.array_equal(got[0].view(np.uint32), base[0].view(np.uint32)), 'an empty scene is the ambient'
        outside = np.broadcast_to(~inside[:, None, :], got.shape)
        assert np.array_equal(got[outside].view(np.uint32), base[outside].view(np.uint32)), 'outside the supports the output is the ambient'
        again = _render_guarded(scenes, pool, bank, amb)
        assert torch.equal(_bits(out), _bits(again)), 'two runs give equal bits'
        for b in (6, 7):
            alone = sc.render_scenes(scenes[b], pool, bank, ambient=None if amb is None else amb[b:b + 1].contiguous())
            assert torch.equal(_bits(alone[0]), _bits(out[b])), 'a clip does not depend on its batch'
        # the torch.fft leg of SALSA_HIP_SCENE=0 meets the same bound and the same exact properties
        monkeypatch.setattr(sc, 'HIP_SCENE', False)
        leg = sc.render_scenes(scenes, pool, bank, ambient=amb).cpu().numpy()
        monkeypatch.setattr(sc, 'HIP_SCENE', True)
        leg_err = float(np.abs(leg.astype(np.float64) - ref).max())
        print('    torch.fft leg: err %.3g, err / Y %.2f' % (leg_err, leg_err / Y))
        assert leg_err <= bound
        assert np.array_equal(leg[outside].view(np.uint32), base[outside].view(np.uint32))


@pytest.mark.parametrize('C', [4, 6])
def test_static_items_through_the_new_entry_point_give_the_old_bits(C):
    """the batch of tests/test_scenes_gpu.py at L = 513 and events of 3000 samples: a static item is ONE segment of step 0, loaded
    without a window and accumulated in the items' order, so salsa_scene_render_moving repeats salsa_scene_render bit for bit"""
    from test_scenes_gpu import _case as static_case
    scenes, pool, bank = static_case(513, 3000, C)
    assert not scenes.has_trajectories
    amb_np = (0.05 * np.random.RandomState(7).randn(scenes.n_clips, C, N)).astype(np.float32)
    for amb in (None, torch.from_numpy(amb_np).cuda()):
        old = _render_guarded(scenes, pool, bank, amb)
        new = _render_guarded(scenes, pool, bank, amb, segments=True)
        assert float(old.abs().max()) > 0.1 and torch.equal(_bits(old), _bits(new))


def test_more_than_256_segments_in_one_clip():
    """one 3000-sample item at S = 240 (14 segments) among 300 one-sample static items: more than salsa_scene_render's 256 items"""
    from salsa_amd import scenes as sc
    rng = np.random.RandomState(256)
    pool = sc.EventPool([rng.randn(3000).astype(np.float32) * 0.3, np.array([0.5], np.float32)], [0, 1])
    h = rng.randn(4, 4, 513) * 10.0 ** (-2.0 * np.arange(513) / 513)
    bank = sc.RirBank(h.astype(np.float32), [10, -60, 120, -170], [0, 20, -30, 45], 'foa')
    clicks = [(1, int(r), int(o), float(g), 1) for r, o, g in zip(rng.randint(0, 4, 300), np.sort(rng.randint(0, N, 300)), rng.uniform(0.2, 1.0, 300))]
    items = clicks[:150] + [(0, _traj(3000, 240, 0), 900, 1.0, 0)] + clicks[150:]
    scenes = sc.Scenes.from_items(N, [[], items], pool, bank, traj_step=240)
    assert np.diff(sc.segment_tables(scenes, pool, bank)[0]).tolist() == [0, 314]
    amb = (0.05 * rng.randn(2, 4, N)).astype(np.float32)
    ref = mr.render64_moving(scenes, pool, bank, N, amb)
    Y, errs = mr.float32_yardstick(scenes, pool, bank, N, amb, ref)
    out = _render_guarded(scenes, pool, bank, torch.from_numpy(amb).cuda())
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print('314 segments: err %.3g, Y %.3g, err / Y %.2f' % (err, Y, err / Y))
    assert err <= 4.0 * Y + sr.ulp32(np.abs(ref).max())
    assert np.array_equal(got[0].view(np.uint32), amb[0].view(np.uint32))
    assert torch.equal(_bits(out), _bits(_render_guarded(scenes, pool, bank, torch.from_numpy(amb).cuda())))


def test_a_moving_anechoic_foa_item_end_to_end(oracle):
    """render on the device, extract with SalsaExtractor; against the oracle's features of the float64 render.  The bar is that of
    tests/test_scenes_gpu.py::test_an_anechoic_foa_item_puts_its_label_into_every_bin: 1e-5, the feature path's parity bar to the
    oracle, plus 4 x 2.0e-6 for the renderer; the non-zero bins must reach 0.9 x the oracle's count."""
    from salsa_amd import scenes as sc
    from salsa_amd.extractor import SalsaExtractor
    from salsa_amd.synth import _ar1
    pool = sc.EventPool([(0.1 * _ar1(np.random.RandomState(3).randn(24000))).astype(np.float32)], [2])
    bank = sc.make_rir_bank('foa', [(10 * j - 180, 20) for j in range(36)], 64)
    traj = [(3 + k) % 36 for k in range(11)]
    scenes = sc.Scenes.from_items(48000, [[(0, traj, 9137, 0.8, 0)]], pool, bank, traj_step=2400)
    audio = sc.render_scenes(scenes, pool, bank)
    feat = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device('cuda:0')).extract(audio)[0].cpu().numpy()
    ref_feat = oracle.extract_salsa(mr.render64_moving(scenes, pool, bank, 48000)[0].astype(np.float32), audio_format='foa', fmax_doa=9000)
    nz, ref_nz = (feat[4:] != 0).any(axis=0), (ref_feat[4:] != 0).any(axis=0)
    both = nz & ref_nz
    dev = np.abs(feat[4:][:, both] - ref_feat[4:][:, both]).max()
    print('%d non-zero bins (oracle on the float64 render: %d, in both: %d), largest deviation %.3g' % (nz.sum(), ref_nz.sum(), both.sum(), dev))
    assert dev <= 1e-5 + 4 * 2.0e-6
    assert nz.sum() >= 0.9 * ref_nz.sum() and both.sum() >= 0.9 * ref_nz.sum() and ref_nz.sum() > 10000
    # ... and the direction it carries does move: the first and the last node's labels, half a second in and before the end
    for k in (1, 9):
        t = int(round((9137 + 2400 * k) / 300))
        x, y, z = sc._unit(bank.azimuth[traj[k]], 20)
        v = feat[4:, t, nz[t]]
        assert np.median(np.degrees(np.arccos(np.clip(np.array([y, z, x]) @ v / np.linalg.norm(v, axis=0), -1, 1)))) <= 9.4 / 4


@pytest.mark.parametrize('fmt', ['classwise', 'trackwise'])
def test_add_scenes_with_moving_items_feeds_the_bank_and_a_training_step(fmt):
    from salsa_amd import scenes as sc
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor
    NC, n_samples = 12, 8 * 24000
    pool = sc.synth_event_pool(NC, 2, 1, max_s=1.2)
    rbank = sc.make_rir_bank('foa', [(a, e) for a in range(-170, 180, 20) for e in (-30, 10)], 1200, rt60=0.3, seed=2)
    scenes = sc.draw_scenes(2, pool, rbank, n_samples, 4, max_polyphony=3, allow_same_class=(fmt == 'trackwise'), gap_s=(0.1, 0.8),
                            moving=1.0, speed_deg_s=(40.0, 90.0))
    assert scenes.has_trajectories and np.all(np.diff(scenes.traj_start) >= 1)
    rows = sc.scene_rows(scenes[0])
    assert len({(r[1], r[2], r[3]) for r in rows}) > len({(r[1], r[2]) for r in rows})          # directions do change inside events
    ex = SalsaExtractor(audio_format='foa', fmax_doa=9000, device=torch.device('cuda:0'))
    width = NC * (3 if fmt == 'trackwise' else 1)
    bank = GpuFeatureBank(ex, n_classes=width, label_format=fmt)
    amb = 1e-3 * torch.randn(2, 4, n_samples, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    audio = sc.add_scenes(bank, scenes, pool, rbank, ambient=amb)
    assert tuple(audio.shape) == (2, 4, n_samples) and bank.clip_len == [640, 640]
    bank.fit_scaler()
    bank.finalize()
    for b in range(2):
        sed, doa = sc.scene_labels(scenes[b], 80, NC, fmt)
        assert sed.sum() > 0
        assert np.array_equal(bank.sed_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), sed.view(np.uint32))
        assert np.array_equal(bank.doa_all[80 * b:80 * (b + 1)].cpu().numpy().view(np.uint32), doa.view(np.uint32))
    x, sed, doa, names = bank.batch([0, 1])
    assert tuple(x.shape) == (2, 7, 640, 200) and tuple(sed.shape) == (2, 80, width) and tuple(doa.shape) == (2, 80, 3 * width)
    tr = Trainer('cuda', seed=3, **(dict(output_format='multi_accdoa', n_classes=NC) if fmt == 'trackwise' else {}))
    losses = tr.train_step(x, sed, doa)
    assert all(bool(torch.isfinite(v)) for v in losses)
