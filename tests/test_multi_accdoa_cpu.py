"""CPU tests of the Multi-ACCDOA output format: the trackwise label loader, the per-item arithmetic of
salsa_nn_adpit_loss / salsa_nn_seld_decode_multi (salsa_amd/csrc/multi_accdoa.h built with g++: tests/hostemu/multi_accdoa_emu.cpp)
against the numpy restatement of tests/multi_accdoa_reference.py, the torch loss against the 13-way formulation of the DCASE 2022
baseline, a CPU bank with trackwise labels, and the plumbing through Trainer / infer_pipelined with its refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import multi_accdoa_reference as ref
from conftest import ROOT


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('multi_accdoa_emu') / 'libmulti_accdoa_emu.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostemu', 'multi_accdoa_emu.cpp')])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.emu_source_of.argtypes = [C.c_int] * 3
    L.emu_adpit.argtypes = [vp, vp, vp, C.c_long, C.c_int, vp, vp, vp]
    L.emu_adpit.restype = None
    L.emu_decode_multi.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_double, vp, vp, vp, vp]
    return L


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits_or_nan(a, b):
    """bit equality, any NaN equal to any NaN (the payload of a NaN is not part of the contract)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------- 1. labels
def write_csv(path, rows):
    with open(path, 'w') as f:
        for r in rows:
            f.write(','.join(str(v) for v in r) + '\n')
    return str(path)


def test_trackwise_labels_without_overlaps_equal_the_classwise_ones(tmp_path):
    from salsa_amd.dataset import load_classwise_gt, load_trackwise_gt
    rng = np.random.default_rng(0)
    rows = []
    for fr in range(40):                                         # different classes overlap, one class never does; a repeated row
        for cl in rng.choice(12, size=rng.integers(0, 4), replace=False):
            rows.append((fr, cl, int(cl) % 5, int(rng.integers(-180, 180)), int(rng.integers(-60, 60))))
    rows.append(rows[3][:3] + (17, -4))                          # a later row of one (frame, class, track): the last one stays
    fn = write_csv(tmp_path / 'a.csv', rows)
    sed_c, doa_c = load_classwise_gt(fn, 320, 12, 8)
    sed, doa, dropped = load_trackwise_gt(fn, 320, 12, 8)
    assert dropped == 0 and sed.shape == (40, 36) and doa.shape == (40, 108) and sed.dtype == doa.dtype == np.float32
    d = doa.reshape(40, 3, 3, 12)                                # (frame, axis, slot, class)
    assert np.array_equal(sed[:, :12], sed_c) and np.array_equal(bits(d[:, :, 0].reshape(40, 36)), bits(doa_c))
    assert not sed[:, 12:].any() and not d[:, :, 1:].any() and sed_c.sum() > 20


def test_trackwise_labels_order_same_class_tracks_by_length(tmp_path):
    from salsa_amd.dataset import load_trackwise_gt
    rows = []
    # class 2: track 0 lasts 9 frames, track 1 6 frames, track 2 6 frames (a tie: the lower id first), track 3 3 frames, track 4 12
    for tr, (lo, hi), azi in ((0, (0, 9), 10), (1, (2, 8), 50), (2, (3, 9), 90), (3, (4, 7), 130), (4, (5, 17), 170)):
        rows += [(fr, 2, tr, azi, 0) for fr in range(lo, hi)]
    rows += [(fr, 5, 0, -30, 20) for fr in range(9, 12)]         # another class on track 0: track 0 has 12 rows, as track 4 has
    fn = write_csv(tmp_path / 'b.csv', rows)
    sed, doa, dropped = load_trackwise_gt(fn, 160, 12, 8)
    d = doa.reshape(20, 3, 3, 12)

    def azimuths(fr):
        return [int(round(np.degrees(np.arctan2(d[fr, 1, n, 2], d[fr, 0, n, 2])))) if sed[fr, n * 12 + 2] else None for n in range(3)]
    assert azimuths(0) == [10, None, None]
    assert azimuths(2) == [10, 50, None]                         # two tracks: the longer first
    assert azimuths(3) == [10, 50, 90]                           # three: 12, 6, 6 rows -- the tie goes to the lower id
    assert azimuths(4) == [10, 50, 90]                           # four: the shortest is dropped
    assert azimuths(5) == [10, 170, 50]                          # five: tracks 0 and 4 tie at 12 rows, then 1; two dropped
    assert azimuths(8) == [10, 170, 90] and azimuths(12) == [170, None, None]
    assert dropped == 1 + 2 + 2 + 1                              # frame 4: track 3; frames 5, 6: tracks 2 and 3; frame 7: track 2
    s = sed.reshape(20, 3, 12)
    assert np.all(s[:, 1] <= s[:, 0]) and np.all(s[:, 2] <= s[:, 1])          # the active slots are a prefix
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    assert np.allclose(norm[s > 0], 1.0, atol=1e-6) and not norm[s == 0].any()


# ---------------------------------------------------------------------------------------------------- 2. the shared header
def test_candidate_tables(emu):
    for k, cands in ref.CANDIDATES.items():
        for ci, cand in enumerate(cands):
            assert tuple(emu.emu_source_of(k, ci, n) for n in range(3)) == cand, (k, ci)


def run_emu_adpit(emu, doa, sed, gt, C_):
    rows = doa.shape[0]
    chosen, item, g = np.zeros((rows, C_), np.uint8), np.zeros((rows, C_), np.float64), np.zeros_like(doa)
    emu.emu_adpit(doa.ctypes.data, sed.ctypes.data, gt.ctypes.data, rows, C_, chosen.ctypes.data, item.ctypes.data, g.ctypes.data)
    return chosen, item, g


@pytest.mark.parametrize('rows,C_,nan', [(1, 1, False), (7, 12, False), (40, 5, True), (64, 14, True)])
def test_hostemu_adpit_equals_the_restatement(emu, rows, C_, nan):
    doa, sed, gt = ref.build_adpit_inputs(rows, C_, seed=rows + C_, nan=nan)
    want = ref.adpit_reference(doa, sed, gt, C_)
    chosen, item, g = run_emu_adpit(emu, doa, sed, gt, C_)
    assert np.array_equal(chosen, want['chosen'])
    assert same_bits_or_nan(item, want['item']) and same_bits_or_nan(g, want['g_doa'])
    if rows >= 40:
        assert set(np.unique(want['k'])) == {0, 1, 2, 3} and len(np.unique(chosen)) == 6 and np.isnan(item).sum() == int(nan)


def test_adpit_ties_and_nan_keep_the_first_candidate(emu):
    """two tracks with one prediction and two slots with one target tie exactly; a NaN cost never displaces an earlier candidate"""
    C_ = 1
    P = np.zeros((4, 1, 3, 3), np.float32)
    T = np.zeros((4, 1, 3, 3), np.float32)
    s = np.zeros((4, 1, 3), bool)
    P[0, 0] = [[1, 0, 0], [1, 0, 0], [0, 1, 0]]                      # k = 2, tracks 0 and 1 equal: 010 ties with 100 -> 010 (index 1)
    T[0, 0, :2], s[0, 0, :2] = [[1, 0, 0], [0, 1, 0]], True          # ... but 001 costs less: 0 0 -> source 0, track 2 -> source 1
    P[1, 0] = [[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]]                # k = 3, all slots one target: the six candidates tie -> 0
    T[1, 0], s[1, 0] = [[0, 0, 1]] * 3, True
    P[2, 0] = [[np.nan, 0, 0], [0, 1, 0], [1, 0, 0]]                 # k = 2, every cost NaN: candidate 0 stays
    T[2, 0, :2], s[2, 0, :2] = [[1, 0, 0], [0, 1, 0]], True
    P[3, 0] = [[0, 1, 0], [1, 0, 0], [0, 1, 0]]                      # slots 0 and 2 active (compaction): best is 101 -> index 4
    T[3, 0, 0], T[3, 0, 2], s[3, 0, 0], s[3, 0, 2] = [1, 0, 0], [0, 1, 0], True, True
    doa, gt = ref.from_items(P), ref.from_items(T)
    sed = np.ascontiguousarray(s.transpose(0, 2, 1)).reshape(4, 3).astype(np.float32)
    chosen, item, g = run_emu_adpit(emu, doa, sed, gt, C_)
    assert chosen.ravel().tolist() == [0, 0, 0, 4] and item[0, 0] == 0.0 and item[3, 0] == 0.0 and np.isnan(item[2, 0])
    want = ref.adpit_reference(doa, sed, gt, C_)
    assert np.array_equal(chosen, want['chosen']) and same_bits_or_nan(g, want['g_doa'])


def run_emu_decode(emu, act, xyz, n_frames, C_, thr, cos_unify):
    rows = np.zeros((3 * n_frames * C_, 4), np.int16)
    n_out, flags, out = np.zeros((n_frames, C_), np.int32), np.zeros((n_frames, C_), np.int32), np.zeros((n_frames, C_, 3, 3), np.float32)
    n = emu.emu_decode_multi(act.ctypes.data, xyz.ctypes.data, n_frames, C_, thr, cos_unify, rows.ctypes.data, n_out.ctypes.data,
                             flags.ctypes.data, out.ctypes.data)
    return rows[:n], n_out, flags, out


@pytest.mark.parametrize('n_in,n_frames,C_,fill', [(1, 1, 1, None), (23, 20, 12, None), (9, 9, 14, 'all'), (5, 5, 3, 'none')])
def test_hostemu_decode_equals_the_restatement_and_the_host_decoder(emu, n_in, n_frames, C_, fill):
    from salsa_amd.crnn.postprocess import cos_unify_of, multi_accdoa_cells, multi_accdoa_rows
    act, xyz = ref.build_decode_inputs(1, n_in, C_, seed=n_in + C_, fill=fill)
    act, xyz = act[0], xyz[0]
    if fill is None and n_in > 1:
        xyz[1, 4 * C_] = np.nan                                    # a NaN component of track 1, class 0, frame 1
    cu = cos_unify_of(15.0)
    want = ref.decode_reference(act, xyz, n_frames, C_, 0.5, cu)
    got = run_emu_decode(emu, act, xyz, n_frames, C_, 0.5, cu)
    host = multi_accdoa_cells(act[:n_frames], xyz[:n_frames], 0.5, cu, C_)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert same_bits_or_nan(got[3], want[3])
    assert np.array_equal(host[0], want[1]) and np.array_equal(host[2], want[2]) and same_bits_or_nan(host[1], want[3])
    rows = multi_accdoa_rows(act, xyz, 0.5, 15.0, C_, n_frames, eval_version='2020', as_array=True)
    assert np.array_equal(rows, want[0].astype(np.int64).reshape(-1, 4))
    rows21 = multi_accdoa_rows(act, xyz, 0.5, 15.0, C_, n_frames)
    assert [r[:2] + r[3:] for r in rows21] == rows.tolist() and all(r[2] == 0 for r in rows21)
    if fill == 'all':
        assert len(rows) == 3 * n_frames * C_
    elif fill == 'none':
        assert len(rows) == 0
    elif n_frames == 20:                                           # every kind of cell is there
        assert {0, 1, 2, 3} <= set(np.unique(want[1])) and {0, 1, 2, 3} <= set(bin(int(f) & 7).count('1') for f in np.unique(want[2]))


def test_decode_at_the_threshold_and_at_the_knife_edge_of_cos_unify(emu):
    from salsa_amd.crnn.postprocess import multi_accdoa_cells
    thr = np.float32(0.3)
    below, above = np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(1))
    for seed in range(6):
        vi, vj, c0 = ref.knife_edge_pair(seed)
        far = (-(vi + vj)).astype(np.float32)
        V = np.stack([vi, vj, far])[None, None]                    # (1 frame, 1 class, track, axis)
        xyz = ref.from_items(V.reshape(1, 1, 3, 3))
        for act3, n_active in (((thr, thr, below), 2), ((above, thr, np.float32(np.nan)), 2), ((thr, below, thr), 2), ((thr, thr, thr), 3)):
            act = np.asarray(act3, np.float32).reshape(1, 3)
            for ulps in (-3, -1, 0, 1, 3):
                cu = c0
                for _ in range(abs(ulps)):
                    cu = float(np.nextafter(cu, -2.0 if ulps < 0 else 2.0))
                want = ref.decode_reference(act, xyz, 1, 1, thr, cu)
                got = run_emu_decode(emu, act, xyz, 1, 1, thr, cu)
                host = multi_accdoa_cells(act, xyz, thr, cu, 1)
                assert np.array_equal(got[0], want[0]) and got[2][0, 0] == want[2][0, 0] == host[2][0, 0] and same_bits_or_nan(got[3], want[3])
                assert same_bits_or_nan(host[1], want[3]) and bin(want[2][0, 0] >> 4).count('1') == n_active
                if act3[1] == thr and act3[0] >= thr and abs(ulps) == 3:                # the pair (0, 1) flips within a few ulps of c0
                    assert bool(want[2][0, 0] & 1) == (ulps < 0)


# ---------------------------------------------------------------------------------------------------- 3. the 13-way formulation
def test_torch_adpit_loss_equals_the_13_way_minimum_with_padding():
    from salsa_amd.crnn.loss import adpit_loss
    C_, rows = 8, 25                                                # 200 items, continuous draws: no ties
    doa, sed, gt = (torch.from_numpy(a) for a in ref.build_adpit_inputs(rows, C_, seed=13, ties=False))
    p1 = doa.clone().reshape(5, 5, 9 * C_).requires_grad_(True)
    logit = torch.randn(5, 5, 3 * C_, requires_grad=True)
    loss, sed_l, doa_l = adpit_loss({'event_frame_logit': logit, 'doa_frame_output': p1}, sed.reshape(5, 5, -1), gt.reshape(5, 5, -1))
    loss.backward()
    p2 = doa.clone().requires_grad_(True)
    want = ref.adpit_13way(p2, sed, gt, C_)
    want.backward()
    exact = ref.adpit_reference(doa.numpy(), sed.numpy(), gt.numpy(), C_)
    assert float(sed_l.detach()) == 0.0 and float(doa_l.detach()) == float(loss.detach()) and loss.dtype == torch.float32
    assert abs(float(loss.detach()) - float(want.detach())) <= 2 * ref.torch_sum_bound(float(want.detach()), rows, C_)
    assert abs(float(loss.detach()) - exact['loss']) <= ref.torch_sum_bound(exact['loss'], rows, C_)
    g1, g2 = p1.grad.reshape(rows, -1).double(), p2.grad
    assert float((g1 - g2).abs().max()) <= 2.0 ** -23 * float(g2.abs().max())   # float32 gradients of a float64 rule
    assert float((g1 - torch.from_numpy(exact['g_doa']).double()).abs().max()) <= 2.0 ** -23 * float(g2.abs().max())
    assert torch.count_nonzero(logit.grad) == 0 and len(np.unique(exact['k'])) == 4


def test_torch_adpit_choice_equals_the_restatement_on_ties_and_nan():
    from salsa_amd.crnn.loss import adpit_choose
    doa, sed, gt = ref.build_adpit_inputs(40, 5, seed=45, nan=True)
    want = ref.adpit_reference(doa, sed, gt, 5)
    cost, chosen, _ = adpit_choose(torch.from_numpy(doa), torch.from_numpy(sed), torch.from_numpy(gt))
    assert np.array_equal(chosen.numpy().astype(np.uint8), want['chosen'])
    item = (torch.gather(cost, 2, chosen[..., None])[..., 0] / 9.0).numpy()
    assert same_bits_or_nan(item, want['item'])


# ---------------------------------------------------------------------------------------------------- 4. the bank
@pytest.mark.parametrize('fmt,ftype', [('foa', 'salsa'), ('mic', 'salsa')])
def test_cpu_bank_with_trackwise_labels_swaps_every_slot(fmt, ftype, tmp_path):
    from salsa_amd import augment as aug
    from salsa_amd.dataset import GpuFeatureBank, load_trackwise_gt
    C_, n_frames, F = 4, 64, 24
    rows = [(fr, cl, tr, 37 * tr + 11 * fr - 100, 9 * tr - 20) for fr in range(8) for cl in (0, 2) for tr in range(1 + (fr + cl) % 3)]
    fns = [write_csv(tmp_path / ('c%d.csv' % i), rows[i:]) for i in range(3)]
    bank = GpuFeatureBank(None, chunk_len_s=32 / 80, chunk_hop_len_s=16 / 80, n_classes=3 * C_, device='cpu', label_format='trackwise')
    feats = torch.randn(3, 7, n_frames, F, generator=torch.Generator().manual_seed(1))
    bank.add_features(feats, ['a', 'b', 'c'], gt_meta=fns)
    bank.finalize(normalize=False)
    sed0, doa0, _ = load_trackwise_gt(fns[0], n_frames, C_, 8)
    assert bank.n_dropped == 0 and torch.equal(bank.sed_all[:8], torch.from_numpy(sed0)) and torch.equal(bank.doa_all[:8], torch.from_numpy(doa0))
    idx = list(range(len(bank)))
    B = len(idx)
    m = torch.zeros((B, 4), dtype=torch.long)
    for b in range(B):
        for k in range(4 if fmt == 'foa' else 3):
            m[b, k] = ((b + 1) >> k) & 1
    zeros = torch.zeros((B, 8), dtype=torch.long)
    d = dict(m=m, shift=torch.zeros(B, dtype=torch.long), up=torch.zeros(B, dtype=torch.bool), u=torch.zeros((B, 8)), top=zeros, h=zeros,
             left=zeros, w=zeros)
    _, sed, doa, _ = bank.batch_augmented(idx, d, fmt, ftype)
    _, s0, d0, _ = bank.batch(idx)
    assert torch.equal(sed, s0) and not torch.equal(doa, d0) and float(s0.reshape(B, -1, 3, C_)[:, :, 2].sum()) > 0
    L = d0.shape[1]
    got, plain = doa.reshape(B, L, 3, 3, C_), d0.reshape(B, L, 3, 3, C_)          # (B, L, axis, slot, class)
    for n in range(3):                                                            # every slot is swap_targets of that slot alone
        want = aug.swap_targets(plain[:, :, :, n].reshape(B, L, 3 * C_), m, fmt, C_)
        assert torch.equal(got[:, :, :, n].reshape(B, L, 3 * C_), want), n


def test_bank_refuses_trackwise_labels_without_three_slots():
    from salsa_amd.dataset import GpuFeatureBank
    with pytest.raises(ValueError, match='three slots'):
        GpuFeatureBank(None, n_classes=14, device='cpu', label_format='trackwise')
    with pytest.raises(ValueError, match='label_format'):
        GpuFeatureBank(None, n_classes=12, device='cpu', label_format='slotwise')
    assert GpuFeatureBank(None, n_classes=14, device='cpu').label_format == 'classwise'


# ---------------------------------------------------------------------------------------------------- 5. plumbing
def pair_batch(batch, n_lab, C_, seed):
    """trackwise labels with same-class pairs: class 0 holds two sources in every frame, class 1 one, class 2 three in some"""
    rng = np.random.default_rng(seed)
    s = np.zeros((batch, n_lab, C_, 3), bool)
    s[:, :, 0, :2] = True
    s[:, :, 1, 0] = True
    s[:, ::3, 2, :] = True
    T = (ref.unit(rng, (batch, n_lab, C_, 3)) * s[..., None]).astype(np.float32)
    sed = np.ascontiguousarray(s.transpose(0, 1, 3, 2)).reshape(batch, n_lab, 3 * C_).astype(np.float32)
    doa = np.ascontiguousarray(T.transpose(0, 1, 4, 3, 2)).reshape(batch, n_lab, 9 * C_)
    return torch.from_numpy(sed), torch.from_numpy(doa)


def test_cpu_trainer_takes_falling_steps_on_same_class_pairs():
    from salsa_amd.crnn.train import OUTPUT_FORMATS, Trainer, synthetic_batch
    assert OUTPUT_FORMATS == ('reg_xyz', 'accdoa', 'multi_accdoa')
    tr = Trainer('cpu', amp_dtype=None, output_format='multi_accdoa', n_classes=12)
    assert tr.n_classes == 12 and tr.raw_model.decoder.n_classes == 36
    ev0 = {k: p.detach().clone() for k, p in tr.raw_model.decoder.event.named_parameters()}
    x, _, _ = synthetic_batch(2, 'cpu', n_frames=64)
    sed, doa = pair_batch(2, 8, 12, seed=2)
    l0 = float(tr.train_step(x, sed, doa)[0])
    loss, sed_l, doa_l = tr.train_step(x, sed, doa)
    assert np.isfinite(l0) and float(loss) < l0 and float(sed_l) == 0.0 and float(doa_l) == float(loss)
    for k, p in tr.raw_model.decoder.event.named_parameters():
        assert torch.count_nonzero(p.grad) == 0 and torch.equal(p.detach(), ev0[k]), k
    act, xyz = tr.infer(x)
    assert act.shape == (2, 8, 36) and xyz.shape == (2, 8, 108)
    assert torch.allclose(act, xyz.reshape(2, 8, 3, 36).norm(dim=2), rtol=1e-6)      # the track activities are the vector lengths


def stub_forward(C_, n_lab):
    """class 1 holds two far-apart tracks in frame 2; class 0 two near-identical ones in frame 0 (unified); nothing else"""
    def forward(x):
        b = x.shape[0]
        V = torch.zeros(b, n_lab, 3, 3, C_)                          # (b, frame, axis, track, class)
        V[:, 2, 0, 0, 1], V[:, 2, 1, 1, 1] = 0.9, 0.8                # tracks 0 and 1 of class 1: +x and +y
        V[:, 0, 0, 0, 0], V[:, 0, 0, 2, 0], V[:, 0, 1, 2, 0] = 0.9, 0.9, 0.05     # tracks 0 and 2 of class 0: 3 degrees apart
        xyz = V.reshape(b, n_lab, 9 * C_)
        return V.norm(dim=2).reshape(b, n_lab, 3 * C_), xyz
    return forward


@pytest.mark.parametrize('chunks', [None, (40, 40), (40, None), (80, 90)])
def test_infer_pipelined_host_returns_two_rows_of_one_class_in_one_frame(chunks):
    from salsa_amd.crnn.infer import infer_clips_sharded, infer_pipelined
    feats = torch.zeros(3, 7, 80, 8)
    kw = dict(sub_batch=2, sed_threshold=0.5, n_label_frames=10, decode='host', output_format='multi_accdoa', n_classes=4, eval_version='2020')
    n_lab = 10
    if chunks:
        kw.update(chunk_len=chunks[0], chunk_hop_len=chunks[1])
        n_lab = chunks[0] // 8
    rows = infer_pipelined(3, lambda lo, hi: feats[lo:hi], stub_forward(4, n_lab), **kw)
    per_chunk = [[0, 0, 2, 0], [2, 1, 0, 0], [2, 1, 90, 0]]         # the unified pair: atan2(0.025, 0.9) = 1.6 degrees -> 2
    want = per_chunk if n_lab == 10 else per_chunk + [[r[0] + 5] + r[1:] for r in per_chunk]
    assert rows == [want] * 3
    out = infer_clips_sharded(['b', 'a', 'c'], lambda ns: feats[:len(ns)], stub_forward(4, n_lab), **kw)
    assert [out[n] for n in 'abc'] == rows


def test_refusals_of_the_format():
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.tta import TtaForward
    feats = torch.zeros(2, 7, 80, 8)
    kw = dict(sub_batch=2, n_label_frames=10, decode='host', output_format='multi_accdoa', n_classes=4)
    calls = []

    def fwd(x):
        calls.append(x.shape)
        return stub_forward(4, x.shape[2] // 8)(x)
    with pytest.raises(ValueError, match='overlap'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, chunk_len=40, chunk_hop_len=20, **kw)
    with pytest.raises(ValueError, match='test-time augmentation'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, tta=('foa', 'salsa'), **kw)
    assert not calls                                               # refused before any forward
    with pytest.raises(ValueError, match='tile'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, chunk_len=48, chunk_hop_len=48, **kw)   # 6 + 6 label frames over 10
    with pytest.raises(ValueError, match='test-time augmentation'):
        TtaForward(fwd, 'foa', 'salsa', output_format='multi_accdoa')
    with pytest.raises(ValueError, match='output_format'):
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, **dict(kw, output_format='polar'))
    with pytest.raises(ValueError, match='expected'):              # a forward of the wrong width
        infer_pipelined(2, lambda lo, hi: feats[lo:hi], fwd, **dict(kw, n_classes=5))


def test_validate_and_fit_pass_the_format_through_and_checkpoints_store_it(tmp_path):
    import inspect
    import types

    from salsa_amd.crnn import adpit_loss, fit  # noqa: F401
    from salsa_amd.crnn.train import Trainer
    assert inspect.signature(fit.validate).parameters['unify_deg'].default == 15.0
    assert inspect.signature(fit.fit).parameters['unify_deg'].default == 15.0
    tr = Trainer('cpu', amp_dtype=None, output_format='multi_accdoa', n_classes=2, decoder_size=32)
    loader = types.SimpleNamespace(seed=5)
    path = str(tmp_path / 'epoch=000.ckpt')
    fit._save(path, tr, loader, 0, 1, dict(steps=[]), None)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    assert ckpt['output_format'] == 'multi_accdoa' and ckpt['n_classes'] == 2
    assert fit._load(path, tr, loader)['epoch'] == 0
    with pytest.raises(ValueError, match='output_format'):
        fit._load(path, Trainer('cpu', amp_dtype=None, output_format='accdoa', n_classes=6, decoder_size=32), loader)
    # a validation pass on the CPU: whole clips through infer_pipelined's host decoder, rows of real classes
    from salsa_amd.dataset import GpuFeatureBank
    bank = GpuFeatureBank(None, chunk_len_s=64 / 80, chunk_hop_len_s=64 / 80, n_classes=6, device='cpu', label_format='trackwise')
    bank.add_features(torch.randn(2, 7, 64, 200, generator=torch.Generator().manual_seed(2)), ['a', 'b'])
    bank.finalize(normalize=False)
    gt = [[(0, 1, 10, 0), (0, 1, 120, 5)], [(3, 0, -50, 0)]]
    val = fit.validate(tr, bank, gt, sed_threshold=0.0, sub_batch=2, return_rows=True)
    assert all(0 <= r[1] < 2 for rows in val['rows'] for r in rows) and len(val['rows'][0]) >= 8 and np.isfinite(val['valSeld'])
    with pytest.raises(ValueError, match='overlap'):
        fit.validate(tr, bank, gt, chunk_len=32, chunk_hop_len=16)
    with pytest.raises(ValueError, match='test-time augmentation'):
        fit.validate(tr, bank, gt, tta=('foa', 'salsa'))


@pytest.fixture(scope='module')
def lib():
    from salsa_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_launchers_refuse_invalid_arguments_before_any_device_call(lib):
    """every call here returns -1 from the host-side checks: nothing is launched, no pointer is read"""
    from salsa_amd import _lib
    assert 'salsa_nn_adpit_loss' in _lib.NN_EXPORTS and 'salsa_nn_seld_decode_multi' in _lib.NN_EXPORTS
    assert os.path.join(ROOT, 'salsa_amd', 'csrc', 'multi_accdoa.hip') in _lib.build_command()
    p = [C.c_void_p(0x10000 * (i + 1)) for i in range(8)]
    good = dict(doa=p[0], sed=p[1], gt=p[2], rows=5, C=12, out3=p[3], g_logit=None, g_doa=p[4], chosen=None, ws=p[5])

    def loss(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_adpit_loss(a['doa'], a['sed'], a['gt'], a['rows'], a['C'], a['out3'], a['g_logit'], a['g_doa'], a['chosen'],
                                       a['ws'], None)
    for bad in (dict(doa=None), dict(sed=None), dict(gt=None), dict(out3=None), dict(g_doa=None), dict(ws=None), dict(rows=0), dict(rows=-3),
                dict(C=0), dict(C=1025), dict(rows=2 ** 31 // (9 * 12) + 1), dict(rows=2 ** 40, C=1)):
        assert loss(**bad) == -1, bad
    good = dict(act=p[0], xyz=p[1], files=2, n_in=45, n_frames=40, C=12, thr=0.5, cu=0.9, rows=p[2], counts=p[3])

    def decode(**kw):
        a = dict(good, **kw)
        return lib.salsa_nn_seld_decode_multi(a['act'], a['xyz'], a['files'], a['n_in'], a['n_frames'], a['C'], a['thr'], a['cu'], a['rows'],
                                              a['counts'], None)
    for bad in (dict(act=None), dict(xyz=None), dict(rows=None), dict(counts=None), dict(rows=C.c_void_p(0x10004)), dict(files=0),
                dict(n_frames=0), dict(n_frames=32768, n_in=40000), dict(n_in=39), dict(C=0), dict(C=32768), dict(n_in=2 ** 20, C=1024),
                dict(cu=float('nan')), dict(cu=1.0000001), dict(cu=-1.5)):
        assert decode(**bad) == -1, bad


def test_device_wrappers_refuse_cpu_tensors():
    from salsa_amd.crnn.decode import decode_multi_rows
    with pytest.raises(ValueError, match='CUDA'):
        decode_multi_rows(torch.zeros(1, 5, 12), torch.zeros(1, 5, 36), n_frames=5, n_classes=4)
    with pytest.raises(ValueError, match='not \\(files'):
        decode_multi_rows(torch.zeros(1, 5, 12), torch.zeros(1, 5, 12), n_frames=5, n_classes=4)
