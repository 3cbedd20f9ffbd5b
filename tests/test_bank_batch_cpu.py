"""CPU tests of the one-call training batch (salsa_bank_batch): the per-element statements of salsa_amd/csrc/bank_batch.h, looped on
the host by tests/hostemu/bank_batch_emu.cpp (g++ -ffp-contract=off), against the composed torch path -- GpuFeatureBank.batch, then
augment.apply_augment_torch, then augment.swap_targets -- bit for bit, for the three recipes; the same file as a stand-alone program
under AddressSanitizer / UBSan on banks allocated at their exact size; the launcher's argument checks; BankLoader's index arithmetic.

Bit equality is exact here: every feature value is a copy, a negation, ONE float32 difference, or lo + (hi - lo) * u in three rounded
float32 operations, and torch's CPU kernels round each of these the same way."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(ROOT, 'tests', 'hostemu', 'bank_batch_emu.cpp')
RECIPE = {'none': 0, 'foa': 1, 'mic': 2, 'gcc': 3}


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('bank_batch_emu') / 'libbank_batch_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so, EMU_SRC])
    L = C.CDLL(so)
    L.emu_bank_batch.restype = C.c_int
    L.emu_bank_batch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    return L


def make_bank(n_channels=7, n_clips=3, n_frames=64, F=24, nc=12, chunk=32, hop=16, seed=0):
    """a CPU bank of seeded features (already 'normalised'): chunks of `chunk` frames at hop `hop`, labels at 1/8 of the frame rate"""
    from salsa_amd.dataset import GpuFeatureBank
    g = torch.Generator().manual_seed(seed)
    bank = GpuFeatureBank(None, fs=24000, hop_len=300, chunk_len_s=chunk / 80, chunk_hop_len_s=hop / 80, n_classes=nc, device='cpu')
    feats = torch.randn(n_clips, n_channels, n_frames, F, generator=g)
    sed = (torch.rand(n_clips, n_frames // 8, nc, generator=g) < 0.3).float()
    doa = torch.randn(n_clips, n_frames // 8, 3 * nc, generator=g) * sed.repeat(1, 1, 3)
    bank.add_features(feats, ['clip%d' % i for i in range(n_clips)], sed=sed.numpy(), doa=doa.numpy())
    return bank.finalize(normalize=False)


def edge_draws(B, T, F, fmt, rects=True):
    """every bit pattern of the swap cycled through the batch, shift 9 up and down, and eight rectangles that overlap, touch all four
    edges and include a full-width stripe"""
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
        if rects:
            d[k][::3] = 0 if k in ('h', 'w') else d[k][::3]      # every third sample has no rectangle at all
    return d


def run_emu(emu, bank, idx, d, recipe, n_zero):
    Cn, n_bank, F = bank.features.shape
    B, T, L, nc = len(idx), bank.chunk_len, bank.chunk_len // bank.upsample, bank.n_classes
    start = np.array([bank.chunk_idx[i] for i in idx], np.int64)
    gt = np.array([bank.gt_idx[i] for i in idx], np.int64)
    par = np.zeros((B, 40), np.int32)
    u = np.zeros((B, 8), np.float32)
    if d is not None:
        par[:, 0:4], par[:, 4], par[:, 5] = d['m'].numpy(), d['shift'].numpy(), d['up'].numpy()
        par[:, 8:16], par[:, 16:24], par[:, 24:32], par[:, 32:40] = (d[k].numpy() for k in ('top', 'h', 'left', 'w'))
        u[:] = d['u'].numpy()
    x, sed, doa = np.empty((B, Cn, T, F), np.float32), np.empty((B, L, nc), np.float32), np.empty((B, L, 3 * nc), np.float32)
    feats, sa, da = (np.ascontiguousarray(t.numpy()) for t in (bank.features, bank.sed_all, bank.doa_all))
    rc = emu.emu_bank_batch(feats.ctypes.data, Cn, n_bank, F, sa.ctypes.data, da.ctypes.data, sa.shape[0], nc, start.ctypes.data,
                            gt.ctypes.data, B, T, L, RECIPE[recipe], n_zero, par.ctypes.data, u.ctypes.data, x.ctypes.data,
                            sed.ctypes.data, doa.ctypes.data)
    assert rc == 0
    return torch.from_numpy(x), torch.from_numpy(sed), torch.from_numpy(doa)


@pytest.mark.parametrize('fmt,ftype,n_channels,nc,F', [('foa', 'linspeciv', 7, 12, 24), ('foa', 'salsa', 7, 14, 25),
                                                      ('mic', 'salsa', 7, 12, 31), ('mic', 'linspecgcc', 10, 14, 24)])
def test_shared_header_equals_the_composed_torch_path(emu, fmt, ftype, n_channels, nc, F):
    from salsa_amd import augment as aug
    bank = make_bank(n_channels=n_channels, F=F, nc=nc)
    swap, _, n_zero, _ = aug.recipe(fmt, ftype)
    # the chunk at frame 0, the chunk that ends on the bank's last frame, overlapping and duplicate chunks; B = 17 > 16 patterns
    idx = ([0, len(bank) - 1, 1, 2, 1, 0] + list(range(len(bank))) * 2)[:17]
    d = edge_draws(len(idx), bank.chunk_len, F, fmt, rects=n_zero is not None)
    x, sed, doa = run_emu(emu, bank, idx, d, swap, n_zero or 0)
    xr, sr, dr, names = bank.batch_augmented(idx, d, fmt, ftype)              # a CPU bank: the composed torch path
    x0, s0, d0, _ = bank.batch(idx)
    xt, yt = aug.apply_augment_torch(x0, d0, d, fmt, nc, ftype)
    assert torch.equal(xr, xt) and torch.equal(dr, yt) and torch.equal(sr, s0) and names == [bank.chunk_name[i] for i in idx]
    assert torch.equal(dr, aug.swap_targets(d0, d['m'], 'foa' if swap == 'foa' else 'mic', nc))
    assert torch.equal(x, xr) and torch.equal(sed, sr) and torch.equal(doa, dr)
    assert not torch.equal(xr, x0) and not torch.equal(dr, d0)               # (the draws do act)


def test_zero_draws_and_clip_batch(emu):
    bank = make_bank(F=25)
    idx = [3, 0, len(bank) - 1]
    x, sed, doa = run_emu(emu, bank, idx, None, 'none', 0)
    x0, s0, d0, names = bank.batch(idx)
    xb, sb, db, nb = bank.batch_augmented(idx)
    assert torch.equal(x, x0) and torch.equal(sed, s0) and torch.equal(doa, d0)
    assert torch.equal(xb, x0) and torch.equal(sb, s0) and torch.equal(db, d0) and nb == names
    assert bank.clip_start == [0, 64, 128] and bank.clip_len == [64, 64, 64]
    clips = bank.clip_batch(1, 3)
    assert torch.equal(clips, torch.stack([bank.features[:, 64:128], bank.features[:, 128:192]]))
    with pytest.raises(IndexError):
        bank.batch_augmented([0, len(bank)])
    with pytest.raises(IndexError):
        bank.batch_augmented([-1])
    with pytest.raises(IndexError):
        bank.clip_batch(2, 4)


def test_clip_batch_refuses_unequal_clips():
    from salsa_amd.dataset import GpuFeatureBank
    bank = GpuFeatureBank(None, chunk_len_s=0.4, chunk_hop_len_s=0.2, device='cpu')
    bank.add_features(torch.zeros(1, 7, 64, 8), ['a'])
    bank.add_features(torch.zeros(1, 7, 96, 8), ['b'])
    bank.finalize(normalize=False)
    with pytest.raises(ValueError):
        bank.clip_batch(0, 2)


def test_sanitizer_program_runs_clean(tmp_path):
    """the stand-alone program (its own main, nothing loaded into python): AddressSanitizer + UBSan over the edge cases on banks
    allocated at their exact size"""
    exe = str(tmp_path / 'bank_batch_emu')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-o', exe, EMU_SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'all edge cases clean' in r.stdout, r.stdout + r.stderr


def test_launcher_refuses_bad_scalars():
    from salsa_amd import _lib
    L = _lib.load()
    assert 'salsa_bank_batch' in _lib.EXPORTS
    p = C.c_void_p(4096)                                                     # never dereferenced: every check precedes the first device call
    good = dict(bank=p, C=7, frames=256, F=200, sed_all=p, doa_all=p, ltot=32, nc=12, start=p, gt=p, B=4, T=64, L=8, recipe=1, nz=0,
                par=p, u=p, rects=0, x=C.c_void_p(8192), sed=p, doa=p, ws=p, stream=None)
    bad = [dict(C=8), dict(recipe=4), dict(recipe=-1), dict(recipe=3), dict(C=10, recipe=2), dict(B=0), dict(B=65536), dict(F=1),
           dict(T=0), dict(T=257), dict(nz=-1), dict(nz=8), dict(par=None), dict(u=None), dict(nc=0), dict(L=0), dict(L=33),
           dict(bank=None), dict(start=None), dict(x=None), dict(sed=None), dict(gt=None), dict(rects=1, ws=None),
           dict(rects=1, recipe=0), dict(T=64, F=1 << 26), dict(x=p)]
    for change in bad:
        a = dict(good, **change)
        assert L.salsa_bank_batch(*a.values()) == _lib.E_INVAL, change
        assert 'salsa_bank_batch' in _lib.last_error()


# ------------------------------------------------------------------------------------------------------- BankLoader
def test_loader_epochs_are_seeded_permutations():
    from salsa_amd.dataset import BankLoader
    bank = make_bank(n_clips=3, n_frames=96)                                  # 5 chunks per clip: 15
    n = len(bank)
    assert n == 15
    ld = BankLoader(bank, batch_size=4, seed=7, augment=False, with_indices=True)
    assert ld.n_batches == 4 and len(ld) == 4
    e0, e1 = ld.epoch_indices(0), ld.epoch_indices(1)
    assert sorted(e0.tolist()) == list(range(n)) and sorted(e1.tolist()) == list(range(n)) and e0.tolist() != e1.tolist()
    assert torch.equal(e0, torch.randperm(n, generator=torch.Generator().manual_seed(7)))
    assert torch.equal(BankLoader(bank, batch_size=4, seed=7).epoch_indices(1), e1)
    assert not torch.equal(BankLoader(bank, batch_size=4, seed=8).epoch_indices(0), e0)
    items = list(ld.epoch(0))
    assert [len(it[4]) for it in items] == [4, 4, 4, 3]                        # the short last batch is kept
    assert torch.equal(torch.cat([it[4] for it in items]), e0)
    x, sed, doa, names = bank.batch(items[3][4].tolist())
    assert torch.equal(items[3][0], x) and torch.equal(items[3][2], doa) and items[3][3] == names
    assert len(BankLoader(bank, batch_size=4, train_fraction=0.6)) == 2        # int(4 * 0.6)
    assert len(list(BankLoader(bank, batch_size=4, train_fraction=0.6, augment=False).epoch(0))) == 2


def test_loader_draws_replay_and_rank_shards():
    from salsa_amd.dataset import BankLoader
    bank = make_bank(n_clips=3, n_frames=96, F=24)
    ld = BankLoader(bank, batch_size=4, seed=3, audio_format='mic', with_indices=True, with_draws=True)
    first, again = list(ld.epoch(2)), list(ld.epoch(2, first_step=2))
    assert len(again) == 2
    for a, b in zip(first[2:], again):                                         # any step can be replayed from (seed, epoch, step)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[5][k], b[5][k]) for k in a[5])
    d = ld.step_draws(2, 1, 4)
    assert all(torch.equal(d[k], first[1][5][k]) for k in d)
    assert any(not torch.equal(first[0][5][k], first[1][5][k]) for k in d)
    world = 4
    shards = [BankLoader(bank, batch_size=2, seed=3, rank=r, world=world) for r in range(world)]
    assert len({len(s) for s in shards}) == 1 and len(shards[0]) == 2            # ceil(15 / 4) = 4 indices per rank, 2 steps each
    per_rank = [s.rank_indices(5) for s in shards]
    assert all(len(p) == 4 for p in per_rank)
    perm = shards[0].epoch_indices(5)
    padded = torch.cat([perm, perm[:1]])
    assert torch.equal(torch.stack(per_rank, dim=1).reshape(-1), padded)       # stride `world`, wrapped: DistributedSampler's split
    assert set(torch.cat(per_rank).tolist()) == set(range(len(bank)))
