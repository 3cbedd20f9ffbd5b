"""CPU tests of training the CRNN on the baseline features (melspeciv, linspeciv: 7 channels; melspecgcc, linspecgcc: 10):
the four augmentation recipes against the reference's own samples (golden g22, tools/make_golden.py), the 10-channel model
against the reference PannResNet22(n_input_channels=10) + SeldDecoder (golden g23, tools/make_golden_crnn10.py), and the
16-channel stem filter layout (include/salsa_nn.h)."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden

BASELINE_TYPES = (('foa', 'linspeciv'), ('foa', 'melspeciv'), ('mic', 'linspecgcc'), ('mic', 'melspecgcc'))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize('fmt,ft', BASELINE_TYPES)
def test_baseline_recipes_reproduce_the_reference_samples(fmt, ft):
    """reference_train_transform(feature_type=...) under np.random.seed(s) = the reference's SeldDataset augmentation of the same
    sample under the same seed (datamodule.py:53-100, dataloader.py:56-60), features and targets bit for bit, 48 seeds per type.
    The aspect ratio comes from the recipe (T / 128 mel, T / 200 linear), not from the fixture."""
    from salsa_amd.augment import reference_train_transform
    meta, a = load_golden('g22_baseline_augment')
    x = torch.from_numpy(a['x10' if ft.endswith('gcc') else 'x7'])
    y_sed, y_doa = torch.from_numpy(a['y_sed']), torch.from_numpy(a['y_doa'])
    changed = 0
    for s, (hx, hd) in zip(meta['seeds'], meta['sha'][ft]):
        np.random.seed(s)
        xo, so, do = reference_train_transform(x, y_sed, y_doa, audio_format=fmt, rng=np.random, feature_type=ft)
        xo, do = xo.numpy(), do.numpy()
        if ('%s_x_%d' % (ft, s)) in a:
            assert np.array_equal(xo, a['%s_x_%d' % (ft, s)]) and np.array_equal(do, a['%s_doa_%d' % (ft, s)])
        assert _sha(xo) == hx, (ft, s)
        assert _sha(do) == hd, (ft, s)
        assert so is y_sed
        changed += not np.array_equal(xo, x.numpy())
    assert changed > len(meta['seeds']) // 2


def test_recipe_table_refuses_what_the_reference_refuses():
    from salsa_amd.augment import augment_batch, draw_augment, recipe, reference_train_transform
    x, sed, doa = torch.zeros(10, 48, 64), torch.zeros(6, 12), torch.zeros(6, 36)
    for fmt, ft in (('foa', 'melspecgcc'), ('foa', 'linspecgcc'), ('mic', 'melspeciv'), ('mic', 'linspeciv'), ('foa', 'salsa_lite')):
        with pytest.raises(NotImplementedError):
            reference_train_transform(x, sed, doa, audio_format=fmt, feature_type=ft)
        with pytest.raises(NotImplementedError):
            draw_augment(2, 48, 64, fmt, feature_type=ft)
        with pytest.raises(NotImplementedError):
            augment_batch(x[None], sed[None], doa[None], fmt, feature_type=ft)
    assert recipe('foa') == ('foa', None, None, 200) and recipe('mic') == ('mic', None, 3, 200)   # the SALSA defaults


def test_gcc_swap_acts_on_the_first_set_bit_and_the_targets_on_every_bit():
    """The reference's mismatch, reproduced (transforms.py:568-614): features take only the first set bit (if / elif / elif),
    targets every set bit (independent ifs, the MIC SALSA target rule)."""
    from salsa_amd.augment import swap_channels_gcc, swap_targets
    g = torch.Generator().manual_seed(4)
    x, doa = torch.randn(8, 10, 5, 16, generator=g), torch.randn(8, 3, 36, generator=g)
    all_bits = torch.ones(8, 3, dtype=torch.long)
    first = torch.tensor([[1, 0, 0]] * 8)
    assert torch.equal(swap_channels_gcc(x, all_bits), swap_channels_gcc(x, first))
    assert not torch.equal(swap_targets(doa, all_bits, 'mic'), swap_targets(doa, first, 'mic'))
    m1 = torch.tensor([[0, 1, 0]] * 8)
    xs = swap_channels_gcc(x, m1)                                     # swap M1 / M4: xc12 <- flip(xc24), xc34 <- flip(xc13)
    assert torch.equal(xs[:, 0], x[:, 3]) and torch.equal(xs[:, 4], x[:, 8].flip(-1)) and torch.equal(xs[:, 9], x[:, 5].flip(-1))
    assert torch.equal(swap_channels_gcc(x, torch.zeros(8, 3, dtype=torch.long)), x)


def test_draw_and_torch_apply_follow_the_recipe():
    """draw_augment / apply_augment_torch for the GCC recipe: the four spectrogram rows shift, the six GCC rows do not; the
    cutout zeroes the GCC rows; the SALSA draws are unchanged by the new argument (same generator -> same draws)."""
    from salsa_amd.augment import apply_augment_torch, draw_augment
    d0 = draw_augment(16, 48, 64, 'mic', torch.Generator().manual_seed(9))
    d1 = draw_augment(16, 48, 64, 'mic', torch.Generator().manual_seed(9), feature_type='salsa')
    assert all(torch.equal(d0[k], d1[k]) for k in d0)
    d = draw_augment(64, 48, 64, 'mic', torch.Generator().manual_seed(9), feature_type='melspecgcc')
    assert int((d['h'] > 0).any(dim=1).sum()) > 8
    x = torch.randn(64, 10, 48, 64, generator=torch.Generator().manual_seed(1)) + 3.0   # no input value is 0
    d['m'].zero_()
    d['h'].zero_()
    xo, _ = apply_augment_torch(x, torch.zeros(64, 6, 36), d, 'mic', feature_type='melspecgcc')
    assert torch.equal(xo[:, 4:], x[:, 4:])
    assert not torch.equal(xo[:, :4], x[:, :4])
    d = draw_augment(64, 48, 64, 'mic', torch.Generator().manual_seed(9), feature_type='melspecgcc')
    d['m'].zero_()
    d['shift'].zero_()
    xo, _ = apply_augment_torch(x, torch.zeros(64, 6, 36), d, 'mic', feature_type='melspecgcc')
    cut = xo[:, 4:] == 0
    assert bool(cut.any()) and torch.equal(cut.all(dim=1), cut.any(dim=1))                    # all six GCC rows or none


def test_ten_channel_model_matches_the_reference_model():
    """SeldCRNN(n_input_channels=10) filled by seeded_fill(.., 7): float32 CPU forward = the reference PannResNet22(10) +
    SeldDecoder (g23) at the tolerance of the 7-channel g9 test; its reference key map lands on the reference model's own keys
    and shapes (conv1 (64, 10, 3, 3)); a 10-channel reference checkpoint loads strictly and reproduces the outputs."""
    from salsa_amd.crnn import SeldCRNN
    from salsa_amd.crnn.testing import seeded_fill
    meta, a = load_golden('g23_crnn10')
    m = SeldCRNN(n_input_channels=10)
    seeded_fill(m, meta['weight_seed'])
    m.eval()
    x = torch.randn(*meta['input_shape'], generator=torch.Generator().manual_seed(meta['input_seed']))
    with torch.no_grad():
        out = m(x)
    np.testing.assert_allclose(out['event_frame_logit'].numpy(), a['event_frame_logit'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out['doa_frame_output'].numpy(), a['doa_frame_output'], rtol=1e-4, atol=1e-5)
    ref = m.reference_state_dict()
    assert {k: list(v.shape) for k, v in ref.items()} == meta['ref_keys']
    assert meta['ref_keys']['encoder.conv_block1.conv1.weight'] == [64, 10, 3, 3]
    m2 = SeldCRNN(n_input_channels=10)
    m2.load_reference_state_dict({'state_dict': {'model.' + k: v.clone() for k, v in ref.items()}})
    m2.eval()
    with torch.no_grad():
        out2 = m2(x)
    assert torch.equal(out2['event_frame_logit'], out['event_frame_logit'])
    with pytest.raises(RuntimeError):
        SeldCRNN().load_reference_state_dict(ref)                     # a 10-channel checkpoint does not fit the 7-channel model


def test_stem_filter_layouts():
    """_stem_filter: Cin <= 8 -> [64][10 taps][8] (unchanged), 9 <= Cin <= 16 -> [64][9 taps][16] = w[co][ci][tap // 3][tap % 3]
    rounded to bf16, ci >= Cin zero (include/salsa_nn.h), against a numpy restatement; with a per-channel scale as well."""
    from salsa_amd.crnn.nn_ops import _stem_filter
    g = torch.Generator().manual_seed(3)
    for cin, shape in ((10, (64, 9, 16)), (16, (64, 9, 16)), (9, (64, 9, 16)), (7, (64, 10, 8)), (8, (64, 10, 8))):
        w = torch.randn(64, cin, 3, 3, generator=g)
        scale = torch.rand(64, generator=g) + 0.5
        for sc in (None, scale):
            wq = _stem_filter(w, sc)
            assert wq.dtype == torch.bfloat16 and tuple(wq.shape) == shape and wq.is_contiguous()
            wn = w.numpy() * (1 if sc is None else sc.numpy()[:, None, None, None])
            want = np.zeros(shape, np.float32)
            for co in range(64):
                for tap in range(9):
                    for ci in range(cin):
                        want[co, tap, ci] = wn[co, ci, tap // 3, tap % 3]
            assert torch.equal(wq, torch.from_numpy(want).to(torch.bfloat16)), (cin, sc is None)


def test_synthetic_batch_channels():
    from salsa_amd.crnn.train import synthetic_batch
    x7, s7, d7 = synthetic_batch(2, 'cpu', seed=5, n_frames=64)
    x, s, d = synthetic_batch(2, 'cpu', seed=5, n_frames=64, n_channels=7)
    assert torch.equal(x, x7) and torch.equal(s, s7) and torch.equal(d, d7)              # the default is the SALSA batch
    x10, _, _ = synthetic_batch(2, 'cpu', seed=5, n_frames=64, n_freq=128, n_channels=10)
    assert tuple(x10.shape) == (2, 10, 64, 128)
