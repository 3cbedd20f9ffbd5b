"""GPU tests of salsa_bank_batch (GpuFeatureBank.batch_augmented / clip_batch on a CUDA bank) against the composed path it replaces:
GpuFeatureBank.batch, then augment.apply_augment_hip, then augment.swap_targets.  Both run the per-element code of
salsa_amd/csrc/bank_batch.h, so every comparison is torch.equal: no tolerance anywhere in this file."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, HOP, FRAMES, CLIPS = 64, 32, 256, 3                                      # 7 chunks per clip, 21 in the bank


def make_bank(n_channels, F, nc, seed=0):
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    bank = GpuFeatureBank(None, fs=24000, hop_len=300, chunk_len_s=T / 80, chunk_hop_len_s=HOP / 80, n_classes=nc, device='cuda')
    feats = torch.randn(CLIPS, n_channels, FRAMES, F, generator=g)
    sed = (torch.rand(CLIPS, FRAMES // 8, nc, generator=g) < 0.3).float()
    doa = torch.randn(CLIPS, FRAMES // 8, 3 * nc, generator=g) * sed.repeat(1, 1, 3)
    bank.add_features(feats, ['clip%d' % i for i in range(CLIPS)], sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize(normalize=False)


def edge_draws(B, F, fmt, rects=True):
    """every bit pattern of the swap cycled through the batch (16 FOA, 8 MIC / GCC), shift 9 up and down, and eight rectangles that
    overlap, touch all four edges and include a full-width stripe"""
    nbits = 4 if fmt == 'foa' else 3
    m = torch.zeros((B, 4), dtype=torch.long)
    for b in range(B):
        for k in range(nbits):
            m[b, k] = (b >> k) & 1
    d = dict(m=m, shift=torch.tensor([(0, 9, 9, 1)[b % 4] for b in range(B)]), up=torch.tensor([b % 3 == 1 for b in range(B)]),
             u=torch.rand((B, 8), generator=torch.Generator().manual_seed(5)))
    geo = dict(top=[0, T - 5, 3, 0, T // 2, 7, T - 1, 2], h=[4, 5, T - 3, T, 3, 9, 1, 6],
               left=[0, F - 7, 0, F - 1, 0, 5, 0, F // 2], w=[6, 7, 3, 1, F, 11, F, 9])
    for k, v in geo.items():
        d[k] = torch.tensor(v).repeat(B, 1) if rects else torch.zeros((B, 8), dtype=torch.long)
        if rects and k in ('h', 'w'):
            d[k][::3] = 0                                                     # every third sample has no rectangle at all
    return d


def composed(bank, idx, d, fmt, ftype):
    from salsa_amd import augment as aug
    x, sed, doa, names = bank.batch(idx)
    swap = aug.recipe(fmt, ftype)[0]
    return (aug.apply_augment_hip(x, d, fmt, ftype), sed,
            aug.swap_targets(doa, d['m'].cuda(), 'foa' if swap == 'foa' else 'mic', bank.n_classes), names)


def spy_on_call(bank, monkeypatch):
    seen = []
    inner = bank._bank_call
    monkeypatch.setattr(bank, '_bank_call', lambda *a: (seen.append(a), inner(*a))[1])
    return seen


CASES = [('foa', 'linspeciv', 7, 12, 200), ('foa', 'salsa', 7, 14, 191), ('mic', 'salsa', 7, 12, 191), ('mic', 'salsa', 7, 14, 128),
         ('mic', 'linspecgcc', 10, 12, 200), ('mic', 'melspecgcc', 10, 14, 128)]


@pytest.mark.parametrize('fmt,ftype,n_channels,nc,F', CASES)
def test_equals_the_composed_path_bit_for_bit(fmt, ftype, n_channels, nc, F, monkeypatch):
    from salsa_amd import augment as aug
    bank = make_bank(n_channels, F, nc)
    n = len(bank)
    assert n == 21
    has_cutout = aug.recipe(fmt, ftype)[2] is not None
    # the chunk at frame 0, the chunk that ends on the bank's last frame, overlapping neighbours, duplicates; B = 33
    idx33 = ([0, n - 1, 1, 2, 1, 0, n - 1] + list(range(n)) * 2)[:33]
    seen = spy_on_call(bank, monkeypatch)
    for idx in (idx33, [n - 1], [0]):                                         # B = 33 and B = 1
        d = edge_draws(len(idx), F, fmt, rects=has_cutout)
        if len(idx) == 1:                                                     # (sample 1 of the pattern: swap bit 0, shift 9 up, rectangles)
            d = {k: v[1:2] for k, v in edge_draws(2, F, fmt, rects=has_cutout).items()}
        x, sed, doa, names = bank.batch_augmented(idx, d, fmt, ftype)
        xr, sr, dr, nr = composed(bank, idx, d, fmt, ftype)
        assert x.shape == (len(idx), n_channels, T, F) and doa.shape == (len(idx), T // 8, 3 * nc)
        assert torch.equal(x, xr) and torch.equal(sed, sr) and torch.equal(doa, dr) and names == nr
    assert len(seen) == 3 and all(call[-2] == has_cutout for call in seen)
    # a batch in which the host drew no rectangle: the min / max launch is skipped
    d = edge_draws(33, F, fmt, rects=False)
    x, sed, doa, _ = bank.batch_augmented(idx33, d, fmt, ftype)
    xr, sr, dr, _ = composed(bank, idx33, d, fmt, ftype)
    assert seen[-1][-2] is False and seen[-1][-1] is None
    assert torch.equal(x, xr) and torch.equal(sed, sr) and torch.equal(doa, dr)
    x0, s0, d0, _ = bank.batch(idx33)
    assert not torch.equal(x, x0) and not torch.equal(doa, d0)


@pytest.mark.parametrize('n_channels,nc,F', [(7, 12, 191), (10, 14, 128)])
def test_zero_draws_clip_batch_and_the_switch(n_channels, nc, F, monkeypatch):
    bank = make_bank(n_channels, F, nc, seed=1)
    fmt, ftype = ('mic', 'salsa') if n_channels == 7 else ('mic', 'linspecgcc')
    idx = [5, 0, 20, 5]
    x0, s0, d0, names = bank.batch(idx)
    seen = spy_on_call(bank, monkeypatch)
    x, sed, doa, nb = bank.batch_augmented(idx, None, fmt, ftype)
    assert torch.equal(x, x0) and torch.equal(sed, s0) and torch.equal(doa, d0) and nb == names
    zero = edge_draws(4, F, 'mic', rects=False)
    zero['m'].zero_(), zero['shift'].zero_()
    x, sed, doa, _ = bank.batch_augmented(idx, zero, fmt, ftype)
    assert torch.equal(x, x0) and torch.equal(sed, s0) and torch.equal(doa, d0)
    clips = bank.clip_batch(1, 3)
    assert torch.equal(clips, torch.stack([bank.features[:, FRAMES:2 * FRAMES], bank.features[:, 2 * FRAMES:]]))
    assert len(seen) == 3
    d = edge_draws(4, F, 'mic')
    fused = bank.batch_augmented(idx, d, fmt, ftype)
    monkeypatch.setenv('SALSA_BANK_BATCH', '0')                               # the one switch: the composed path, no fused call
    off = bank.batch_augmented(idx, d, fmt, ftype)
    assert len(seen) == 4 and all(torch.equal(a, b) for a, b in zip(fused[:3], off[:3]))
    assert torch.equal(bank.clip_batch(1, 3), clips) and len(seen) == 4


def test_the_real_banks_extent():
    """float32 [7][1 920 000][200] = 2.69e9 elements: every offset from channel 5 on is past int32.  Only the windows that are read,
    near the end of every channel, are filled."""
    from salsa_amd import augment as aug
    from salsa_amd.dataset import GpuFeatureBank
    free = torch.cuda.mem_get_info()[0]
    if free < 24 * 2 ** 30:
        print('free device memory: %.2f GB' % (free / 2 ** 30))
        pytest.skip('%.2f GB of device memory free, the 10.75 GB bank test wants 24 GB' % (free / 2 ** 30))
    n_frames, F, chunk = 1_920_000, 200, 640
    bank = GpuFeatureBank(None, chunk_len_s=8.0, device='cuda')
    assert bank.chunk_len == chunk
    big = torch.empty((7, n_frames, F), device='cuda')
    starts = [n_frames - chunk, n_frames - chunk - 1000, n_frames - chunk - 5000]
    g = torch.Generator(device='cuda').manual_seed(3)
    for s in starts:
        big[:, s:s + chunk] = torch.randn((7, chunk, F), device='cuda', generator=g)
    bank.features = big
    bank.sed_all = (torch.rand((n_frames // 8, 12), device='cuda', generator=g) < 0.3).float()
    bank.doa_all = torch.randn((n_frames // 8, 36), device='cuda', generator=g)
    bank.chunk_idx, bank.gt_idx, bank.chunk_name = starts, [s // 8 for s in starts], ['a', 'b', 'c']
    assert (6 * n_frames + starts[0]) * F > 2 ** 31
    idx = [0, 1, 2, 0]
    d = aug.draw_augment(4, chunk, F, 'mic', torch.Generator().manual_seed(11))
    d['m'][:, :3] = torch.tensor([[1, 0, 1], [0, 1, 0], [1, 1, 1], [0, 0, 0]])
    d['h'][:, 0], d['w'][:, 0], d['top'][:, 0], d['left'][:, 0] = 40, 50, 600, 150      # a rectangle in every sample: min / max runs
    x, sed, doa, _ = bank.batch_augmented(idx, d, 'mic', 'salsa')
    x0 = torch.stack([big[:, starts[i]:starts[i] + chunk] for i in idx])
    assert torch.equal(bank.batch_augmented(idx, None, 'mic', 'salsa')[0], x0)
    assert torch.equal(x, aug.apply_augment_hip(x0, d, 'mic', 'salsa'))
    d0 = torch.stack([bank.doa_all[starts[i] // 8:starts[i] // 8 + 80] for i in idx])
    assert torch.equal(doa, aug.swap_targets(d0, d['m'].cuda(), 'mic', 12))
    assert torch.equal(sed, torch.stack([bank.sed_all[starts[i] // 8:starts[i] // 8 + 80] for i in idx]))
