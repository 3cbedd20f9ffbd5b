"""GPU tests of Trainer.fit on the bf16 HIP path: 4 clips x 256 frames x 200 bins read from feature files, chunks of 128 frames at hop
64 (12 chunks), batch 5 (steps of 5, 5 and 2 chunks), the MIC SALSA recipe (swaps, shifts and cutouts through salsa_bank_batch) and 2
validation clips.  Weights are compared with torch.equal: the training step is deterministic in its default setting, so the same seed
gives the same bits, a resumed run repeats the uninterrupted one, and the fused batch call changes nothing against the composed path.
The one tolerance is the device scorer's own: total_DE within DE_TP x crnn.score.DEFAULT_MARGIN of the host's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FRAMES, F, CHUNK, HOP, NC = 256, 200, 128, 64, 12
SCHEDULE = dict(milestones=(0.0, 0.1, 0.7, 1.0), lrs=(3e-4, 3e-4, 3e-4, 1e-4), moms=(0.95, 0.85, 0.9, 0.99))
CONSTANT = dict(milestones=(0.0, 0.1, 0.7, 1.0), lrs=(3e-4, 3e-4, 3e-4, 3e-4), moms=(0.9, 0.9, 0.9, 0.9))


def bank_from_files(tmp, n_clips, seed):
    from salsa_amd import io as sio
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    files = [sio.save_arrays(str(tmp / ('s%d_clip%d.h5' % (seed, i))), feature=torch.randn(7, FRAMES, F, generator=g).numpy())
             for i in range(n_clips)]
    sed = (torch.rand(n_clips, FRAMES // 8, NC, generator=g) < 0.2).float()
    v = torch.randn(n_clips, FRAMES // 8, 3, NC, generator=g)
    doa = ((v / v.norm(dim=2, keepdim=True)) * sed[:, :, None, :]).reshape(n_clips, FRAMES // 8, 3 * NC)
    bank = GpuFeatureBank(None, chunk_len_s=CHUNK / 80, chunk_hop_len_s=HOP / 80, n_classes=NC, device='cuda')
    bank.set_scaler(np.zeros((4, 1, F), np.float32), np.ones((4, 1, F), np.float32))
    bank.add_feature_files(files, sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize()


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('fit_gpu')
    bank, val_bank = bank_from_files(tmp, 4, 0), bank_from_files(tmp, 2, 9)
    assert len(bank) == 12 and val_bank.clip_len == [FRAMES, FRAMES]
    rng = np.random.RandomState(4)
    gt = [[(f, int(rng.randint(NC)), int(rng.randint(-180, 180)), int(rng.randint(-40, 40)), 0) for f in range(0, FRAMES // 8, 2)]
          for _ in range(2)]
    return tmp, bank, val_bank, gt


def run(data, out, seed=5, trainer_seed=11, **kw):
    from salsa_amd.crnn.train import Trainer
    tmp, bank, val_bank, gt = data
    tr = Trainer('cuda', seed=trainer_seed)
    args = dict(val_bank=val_bank, val_gt=gt, batch_size=5, max_epochs=2, seed=seed, audio_format='mic', out_dir=str(tmp / out), **SCHEDULE)
    args.update(kw)
    return tr, tr.fit(bank, **args)


def same_weights(a, b):
    sa, sb = a.raw_model.state_dict(), b.raw_model.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.fixture(scope='module')
def full(data):
    return run(data, 'full')


def test_same_seed_same_bits(data, full):
    tr, hist = full
    assert len(hist['steps']) == 6 and len(hist['val']) == 2 and hist['best'] is not None
    again, hist2 = run(data, 'again')
    assert same_weights(tr, again) and hist2['steps'] == hist['steps'] and hist2['val'] == hist['val']
    other, _ = run(data, 'other', seed=6)                                     # (another permutation and other draws: other weights)
    assert not same_weights(tr, other)


def test_resume_equals_the_uninterrupted_run(data, full):
    import os
    tr, hist = full
    _, h1 = run(data, 'sliced', epochs=1)
    assert h1['epoch'] == 1 and os.listdir(str(data[0] / 'sliced' / 'checkpoint')) == ['epoch=000.ckpt']
    resumed, h2 = run(data, 'sliced', trainer_seed=77, resume=True)
    assert h2['epoch'] == 2 and os.listdir(str(data[0] / 'sliced' / 'checkpoint')) == ['epoch=001.ckpt']
    assert same_weights(tr, resumed) and h2['steps'] == hist['steps'] and h2['val'] == hist['val']
    assert sorted(os.listdir(str(data[0] / 'sliced' / 'best'))) == sorted(os.listdir(str(data[0] / 'full' / 'best')))


def test_fit_equals_the_hand_loop(data):
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import BankLoader
    _, bank, _, _ = data
    fitted, hist = run(data, 'hand', max_epochs=1, augment=False, val_bank=None, val_gt=None, **CONSTANT)
    hand = Trainer('cuda', seed=11)
    perm = BankLoader(bank, batch_size=5, seed=5).epoch_indices(0)
    losses = []
    for step in range(3):
        x, sed, doa, _ = bank.batch(perm[step * 5:(step + 1) * 5].tolist())
        losses.append(torch.stack(hand.train_step(x, sed, doa)))              # lr_at: progress < 0.7, exactly 3e-4
    assert same_weights(fitted, hand)
    assert torch.stack(losses).cpu().tolist() == [list(s[4:]) for s in hist['steps']]


def test_the_switch_gives_the_same_weights(data, full, monkeypatch):
    monkeypatch.setenv('SALSA_BANK_BATCH', '0')
    composed, hist = run(data, 'composed')
    assert same_weights(full[0], composed) and hist['steps'] == full[1]['steps']


def test_validation_numbers_against_the_host_scorer(data, full):
    from salsa_amd.crnn.fit import validate
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    tr, hist = full
    _, _, val_bank, gt = data
    val = validate(tr, val_bank, gt, chunk_len=CHUNK, chunk_hop_len=HOP)
    dev = val['scorer']
    rows = infer_pipelined(2, val_bank.clip_batch, tr.infer, n_label_frames=FRAMES // 8, decode='device', chunk_len=CHUNK,
                           chunk_hop_len=HOP, sub_batch=1, eval_version='2020')     # (4-column rows)
    assert sum(len(r) for r in rows) > 0                                      # a fresh model's activities are near 0.5, above 0.3
    host = SeldMetrics(NC, 20)
    for pred, g in zip(rows, gt):
        host.update(pred, g, max_frames=FRAMES // 8, label_rate=10)
    for name in ('TP', 'FP', 'FN', 'S', 'D', 'I', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN'):
        assert getattr(dev, name) == getattr(host, name), name
    print('total_DE device %r host %r, DE_TP %d' % (dev.total_DE, host.total_DE, host.DE_TP))
    assert abs(dev.total_DE - host.total_DE) <= host.DE_TP * DEFAULT_MARGIN
    ER, F1, LE, LR = host.scores()
    assert (val['valER'], val['valF1'], val['valLR']) == (ER, F1, LR)
    assert abs(val['valLE'] - LE) <= DEFAULT_MARGIN
    # what fit recorded after the last epoch is this pass over whole clips (its default test chunk)
    whole = validate(tr, val_bank, gt)
    assert {k: whole[k] for k in ('valER', 'valF1', 'valLE', 'valLR', 'valSeld')} == {k: hist['val'][-1][k] for k in whole if k != 'scorer'}
