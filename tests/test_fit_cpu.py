"""CPU tests of crnn/fit.py: the step-indexed schedule against the reference's LearningRateScheduler (golden g30, written by
tools/make_golden_fit.py), Trainer.fit on Trainer('cpu', amp_dtype=None) against a hand loop of bank.batch + train_step, the
checkpoint names against the three parsing rules of the reference's experiments/inference.py:49-63, resuming, and n_classes = 14.

Equality with the hand loop is asked bit for bit, with torch's CPU kernels run to run taken into account: the hand loop runs twice,
and `fit` may differ from it by at most four times the largest difference between those two runs (measured here: 0.0 -- torch's CPU
kernels repeated themselves exactly on every run of this file, so the assertion is torch.equal in effect)."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANT = dict(milestones=(0.0, 0.1, 0.7, 1.0), lrs=(3e-4, 3e-4, 3e-4, 3e-4), moms=(0.9, 0.9, 0.9, 0.9))


@pytest.fixture(scope='module')
def g30():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'g30_fit.npz'))
    return json.loads(str(z['meta'])), z


def test_schedule_equals_the_reference_at_every_recorded_step(g30):
    from salsa_amd.crnn.fit import lr_mom_at_step
    meta, z = g30
    assert [s['name'] for s in meta['schedules']] == ['shipped_50x1313', 'short_3x3', 'odd_7x13', 'short_2x5']
    for k, s in enumerate(meta['schedules']):
        lr, mom = z['s%d_lr' % k], z['s%d_mom' % k]
        assert len(lr) == s['max_epochs'] * s['steps_per_epoch']
        steps = range(len(lr)) if len(lr) < 1000 else list(range(0, len(lr), 97)) + list(range(6560, 6570)) + list(range(45950, 45960)) \
            + [len(lr) - 1]
        for i in steps:
            got = lr_mom_at_step(i, s['steps_per_epoch'], s['max_epochs'], s['milestones'], s['lrs'], s['moms'])
            assert got == (lr[i], mom[i]), (s['name'], i)
    assert len({float(m) for m in z['s1_mom']}) > 3                           # (non-constant momenta were recorded)


def test_short_schedule_differs_from_lr_at(g30):
    """3 x 3 steps: the reference's step milestones are int(0.7 * 9) = 6 and 9, so step 7 is a third of the way down (2.33e-4);
    lr_at(7 / 9) interpolates from progress 0.7 (2.48e-4).  At the shipped 50 x 1313 the two agree."""
    from salsa_amd.crnn.fit import lr_mom_at_step
    from salsa_amd.crnn.train import lr_at
    _, z = g30
    ref = float(z['s1_lr'][7])
    assert lr_mom_at_step(7, 3, 3)[0] == ref and abs(ref - 2.3333e-4) < 1e-8
    assert abs(lr_at(7 / 9) - 2.4815e-4) < 1e-8 and abs(lr_at(7 / 9) - ref) > 1e-5
    n = 50 * 1313
    for i in (0, 6565, 45954, 45955, 50000, n - 1):
        assert abs(lr_at(i / n) - float(z['s0_lr'][i])) < 1e-12


# ------------------------------------------------------------------------------------------------------- fit
F, CHUNK, FRAMES = 32, 64, 128


def make_bank(n_clips, nc=12, seed=0, hop=32):
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    bank = GpuFeatureBank(None, chunk_len_s=CHUNK / 80, chunk_hop_len_s=hop / 80, n_classes=nc, device='cpu')
    feats = torch.randn(n_clips, 7, FRAMES, F, generator=g)
    sed = (torch.rand(n_clips, FRAMES // 8, nc, generator=g) < 0.2).float()
    v = torch.randn(n_clips, FRAMES // 8, 3, nc, generator=g)
    doa = ((v / v.norm(dim=2, keepdim=True)) * sed[:, :, None, :]).reshape(n_clips, FRAMES // 8, 3 * nc)
    bank.add_features(feats, ['clip%d' % i for i in range(n_clips)], sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize(normalize=False)


def make_gt(n_clips, nc=12):
    """ground-truth rows per clip (frame, class, azimuth, elevation, track), as metrics.load_dcase_csv gives them"""
    rng = np.random.RandomState(4)
    return [[(int(f), int(rng.randint(nc)), float(rng.randint(-180, 180)), float(rng.randint(-40, 40)), 0) for f in range(0, FRAMES // 8, 2)]
            for _ in range(n_clips)]


def hand_loop(bank, n_steps, batch, seed):
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import BankLoader
    tr = Trainer('cpu', amp_dtype=None, seed=11)
    perm = BankLoader(bank, batch_size=batch, seed=seed).epoch_indices(0)
    losses = []
    for step in range(n_steps):
        x, sed, doa, _ = bank.batch(perm[step * batch:(step + 1) * batch].tolist())
        losses.append([float(v) for v in tr.train_step(x, sed, doa)])          # lr_at: every progress < 0.7, exactly 3e-4
    return tr, losses


def max_diff(sd_a, sd_b):
    return max(float((sd_a[k].double() - sd_b[k].double()).abs().max()) for k in sd_a)


def test_fit_equals_the_hand_loop(tmp_path):
    from salsa_amd.crnn.train import Trainer
    bank = make_bank(2)                                                        # 3 chunks per clip: 6 chunks, batch 2 -> 3 steps
    assert len(bank) == 6
    a, losses_a = hand_loop(bank, 3, 2, seed=5)
    b, losses_b = hand_loop(bank, 3, 2, seed=5)
    spread = max_diff(a.raw_model.state_dict(), b.raw_model.state_dict())
    print('hand loop run-to-run spread: %g' % spread)                          # measured: 0
    tr = Trainer('cpu', amp_dtype=None, seed=11)
    hist = tr.fit(bank, batch_size=2, max_epochs=1, augment=False, seed=5, out_dir=str(tmp_path), **CONSTANT)
    assert len(hist['steps']) == 3 and hist['epoch'] == 1 and hist['global_step'] == 3
    assert [s[:4] for s in hist['steps']] == [(0, i, 3e-4, 0.9) for i in range(3)]
    assert max_diff(tr.raw_model.state_dict(), a.raw_model.state_dict()) <= 4 * spread
    loss_spread = max(abs(p - q) for r, s in zip(losses_a, losses_b) for p, q in zip(r, s))
    assert max(abs(p - q) for r, s in zip(losses_a, hist['steps']) for p, q in zip(r, s[4:])) <= 4 * loss_spread
    ckpt = torch.load(str(tmp_path / 'checkpoint' / 'epoch=000.ckpt'), weights_only=False)
    assert ckpt['epoch'] == 0 and ckpt['global_step'] == 3 and ckpt['loader_seed'] == 5 and ckpt['rng_cpu'] is not None
    assert any(k.startswith('encoder.conv_block1.') for k in ckpt['state_dict'])   # the reference's key names
    assert not os.path.exists(str(tmp_path / 'best'))                         # no validation: no best checkpoint


def test_checkpoint_names_resume_and_best(tmp_path):
    from salsa_amd.crnn.train import Trainer
    bank, val_bank, gt = make_bank(2), make_bank(2, seed=9), make_gt(2)
    kw = dict(val_bank=val_bank, val_gt=gt, batch_size=3, max_epochs=3, seed=5, audio_format='foa', out_dir=str(tmp_path),
              milestones=(0.0, 0.1, 0.7, 1.0), lrs=(3e-4, 3e-4, 3e-4, 1e-4), moms=(0.95, 0.85, 0.9, 0.99), val_interval=1)
    full = Trainer('cpu', amp_dtype=None, seed=11)
    hist = full.fit(bank, **kw)
    assert len(hist['steps']) == 6 and [v['epoch'] for v in hist['val']] == [0, 1, 2]
    from salsa_amd.crnn.fit import lr_mom_at_step
    assert [s[2:4] for s in hist['steps']] == [lr_mom_at_step(i, 2, 3, kw['milestones'], kw['lrs'], kw['moms']) for i in range(6)]
    assert os.listdir(str(tmp_path / 'checkpoint')) == ['epoch=002.ckpt']      # the latest only
    best = os.listdir(str(tmp_path / 'best'))
    assert len(best) == 1
    # experiments/inference.py:49-63: startswith('epoch') / endswith('ckpt'); int(f[6:9]) is the epoch; the SECOND number is valSeld
    name = best[0]
    assert name.startswith('epoch') and name.endswith('ckpt')
    assert int(name[6:9]) == hist['best']['epoch']
    numbers = re.findall(r"[-+]?\d*\.\d+|\d+", name)
    assert float(numbers[1]) == float('%.3f' % hist['best']['valSeld'])
    assert len(numbers) == 7 and numbers[3] == '1'                             # (epoch, five scores, and the 1 of 'valF1')
    assert hist['best']['valSeld'] == min(v['valSeld'] for v in hist['val'])
    for v in hist['val']:
        assert set(v) == {'valER', 'valF1', 'valLE', 'valLR', 'valSeld', 'epoch'}
        assert v['valSeld'] == (v['valER'] + 1 - v['valF1'] + v['valLE'] / 180 + 1 - v['valLR']) / 4
    assert int('epoch=002.ckpt'[6:9]) == 2
    # time-sliced: one epoch, then resume to the end -- the same weights as the uninterrupted run
    part_dir = tmp_path / 'sliced'
    first = Trainer('cpu', amp_dtype=None, seed=11)
    h1 = first.fit(bank, **dict(kw, out_dir=str(part_dir), epochs=1))
    assert h1['epoch'] == 1 and os.listdir(str(part_dir / 'checkpoint')) == ['epoch=000.ckpt']
    second = Trainer('cpu', amp_dtype=None, seed=77)                           # (its own initialisation is overwritten by the checkpoint)
    h2 = second.fit(bank, **dict(kw, out_dir=str(part_dir), resume=True))
    assert h2['epoch'] == 3 and len(h2['steps']) == 6 and os.listdir(str(part_dir / 'checkpoint')) == ['epoch=002.ckpt']
    again = Trainer('cpu', amp_dtype=None, seed=11)
    again.fit(bank, **dict(kw, out_dir=str(tmp_path / 'again')))
    spread = max_diff(full.raw_model.state_dict(), again.raw_model.state_dict())
    print('fit run-to-run spread: %g' % spread)                                # measured: 0
    assert max_diff(second.raw_model.state_dict(), full.raw_model.state_dict()) <= 4 * spread
    assert [s[:4] for s in h2['steps']] == [s[:4] for s in hist['steps']]
    # mode 'eval' keeps no best file; a bad mode and validation clips of unequal length are refused
    ev = Trainer('cpu', amp_dtype=None, seed=11)
    ev.fit(bank, **dict(kw, out_dir=str(tmp_path / 'eval'), mode='eval', max_epochs=1))
    assert not os.path.exists(str(tmp_path / 'eval' / 'best'))
    with pytest.raises(ValueError):
        ev.fit(bank, mode='test')


def test_validation_refuses_unequal_clips():
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    val = GpuFeatureBank(None, chunk_len_s=CHUNK / 80, chunk_hop_len_s=0.4, device='cpu')
    val.add_features(torch.zeros(1, 7, 128, F), ['a'])
    val.add_features(torch.zeros(1, 7, 192, F), ['b'])
    val.finalize(normalize=False)
    with pytest.raises(ValueError):
        Trainer('cpu', amp_dtype=None).fit(make_bank(1), val_bank=val, val_gt=[[], []], max_epochs=1)


def test_fourteen_classes_train_a_step():
    from salsa_amd.crnn.train import Trainer
    bank = make_bank(1, nc=14)
    tr = Trainer('cpu', amp_dtype=None, n_classes=14)
    assert tr.raw_model.decoder.n_classes == 14
    x, sed, doa, _ = bank.batch([0, 1])
    assert sed.shape == (2, CHUNK // 8, 14) and doa.shape == (2, CHUNK // 8, 42)
    loss, _, _ = tr.train_step(x, sed, doa, lr=1e-4, beta1=0.8)
    assert torch.isfinite(loss)
    assert tr.opt.param_groups[0]['lr'] == 1e-4 and tr.opt.param_groups[0]['betas'] == (0.8, 0.999)
    hist = tr.fit(bank, batch_size=2, max_epochs=1, train_fraction=0.5, augment=True, audio_format='mic', **CONSTANT)
    assert len(hist['steps']) == 1                                             # int(2 batches * 0.5)
