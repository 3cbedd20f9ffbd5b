"""GPU tests of the Multi-ACCDOA output format: salsa_nn_adpit_loss and salsa_nn_seld_decode_multi through their
C entry points against the numpy restatement of tests/multi_accdoa_reference.py and the host decoder, inside guard bands, and a
Trainer(output_format='multi_accdoa') end to end -- fused against torch loss, a bf16 step from a trackwise bank through
salsa_bank_batch, and infer_pipelined with the rows decoded and scored on the device.

Bounds.  chosen, g_doa, rows and counts are EQUAL to the reference (the same float64 / float32 statements without fma; the decoder's
inputs keep every angle 1e-6 degrees off a rounding edge, a condition on the inputs).  The loss lies within ref.loss_bound of the
exactly rounded sum: the rounding count of the kernel's partial-sum order."""
import ctypes as C

import numpy as np
import pytest
import torch

import multi_accdoa_reference as ref
import seld_score_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GUARD = 64


def ptr(a):
    return C.c_void_p(a.data_ptr()) if a is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def guarded(n, dtype, fill):
    """a buffer of n elements between two guard bands, all filled with `fill` -> (whole, view of the middle)"""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def guards_untouched(whole, fill):
    g = torch.cat([whole[:GUARD], whole[-GUARD:]]).cpu()
    return bool(torch.isnan(g).all()) if isinstance(fill, float) and fill != fill else bool((g == fill).all())


def same_bits_or_nan(a, b):
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------- 1. the loss
def run_loss(doa, sed, gt, C_, g_logit=True, chosen=True):
    from salsa_amd import _lib
    rows = doa.shape[0]
    d, s, t = (torch.from_numpy(a).to(DEV) for a in (doa, sed, gt))
    nan = float('nan')
    bufs = dict(out=guarded(3, torch.float32, nan), gd=guarded(rows * 9 * C_, torch.float32, nan), ws=guarded(64, torch.float64, nan))
    if g_logit:
        bufs['gl'] = guarded(rows * 3 * C_, torch.float32, nan)
    if chosen:
        bufs['ch'] = guarded(rows * C_, torch.uint8, 0xEE)
    mid = {k: v[1] for k, v in bufs.items()}
    rc = _lib.load().salsa_nn_adpit_loss(ptr(d), ptr(s), ptr(t), rows, C_, ptr(mid['out']), ptr(mid.get('gl')), ptr(mid['gd']),
                                         ptr(mid.get('ch')), ptr(mid['ws']), stream())
    assert rc == 0
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        assert guards_untouched(whole, 0xEE if k == 'ch' else nan), k
    return {k: v.cpu().numpy() for k, v in mid.items()}


@pytest.mark.parametrize('rows,C_', [(1, 1), (7, 12), (257, 14), (2560, 12), (3, 1024)])
def test_adpit_loss_kernel_equals_the_restatement(rows, C_):
    doa, sed, gt = ref.build_adpit_inputs(rows, C_, seed=rows + C_)
    want = ref.adpit_reference(doa, sed, gt, C_)
    got = run_loss(doa, sed, gt, C_)
    n_ch = int((got['ch'].reshape(rows, C_) != want['chosen']).sum())
    n_g = int((got['gd'].view(np.uint32) != want['g_doa'].ravel().view(np.uint32)).sum())
    err, bound = abs(float(got['out'][0]) - want['loss']), ref.loss_bound(want['loss'], rows, C_)
    print('adpit (%d, %d): %d chosen differ, %d gradient elements differ, loss %.9g err %.3g / bound %.3g'
          % (rows, C_, n_ch, n_g, want['loss'], err, bound))
    assert n_ch == 0 and n_g == 0
    assert err <= bound and got['out'][2] == got['out'][0] and got['out'][1] == 0.0
    assert not got['gl'].any() and not np.isnan(got['gl']).any()
    again = run_loss(doa, sed, gt, C_)
    assert all(np.array_equal(got[k], again[k]) for k in ('out', 'gd', 'ch', 'gl'))      # fixed-order sums: bit-reproducible
    bare = run_loss(doa, sed, gt, C_, g_logit=False, chosen=False)                       # the optional buffers change nothing else
    assert np.array_equal(bare['out'], got['out']) and np.array_equal(bare['gd'], got['gd'])


def test_adpit_loss_kernel_with_a_nan_prediction():
    doa, sed, gt = ref.build_adpit_inputs(40, 5, seed=45, nan=True)
    want = ref.adpit_reference(doa, sed, gt, 5)
    got = run_loss(doa, sed, gt, 5)
    assert np.array_equal(got['ch'].reshape(40, 5), want['chosen']) and same_bits_or_nan(got['gd'], want['g_doa'].ravel())
    assert np.isnan(got['out'][0]) and np.isnan(got['gd']).sum() == 1


def test_adpit_loss_launcher_refusals_write_nothing():
    from salsa_amd import _lib
    whole, out = guarded(3, torch.float32, 7.0)
    p = torch.zeros(9 * 12, device=DEV)
    for rows, C_, ws in ((0, 12, p), (1, 0, p), (1, 1025, p), (1, 12, None)):
        assert _lib.load().salsa_nn_adpit_loss(ptr(p), ptr(p), ptr(p), rows, C_, ptr(out), None, ptr(p), None, ptr(ws), stream()) == -1
    torch.cuda.synchronize()
    assert bool((whole.cpu() == 7.0).all())


# ---------------------------------------------------------------------------------------------------- 2. the decoder
def run_decode(act, xyz, n_frames, C_, thr, cos_unify):
    """one salsa_nn_seld_decode_multi launch -> (rows per file up to its count, counts); guards and the rows behind the counts checked"""
    from salsa_amd import _lib
    files, n_in = act.shape[:2]
    a, x = torch.from_numpy(act).to(DEV), torch.from_numpy(xyz).to(DEV)
    cap = 3 * n_frames * C_
    rows_w, rows = guarded(files * cap * 4, torch.int16, 0x7EEE)
    counts_w, counts = guarded(files, torch.int32, -77)
    rc = _lib.load().salsa_nn_seld_decode_multi(ptr(a), ptr(x), files, n_in, n_frames, C_, float(thr), float(cos_unify), ptr(rows),
                                                ptr(counts), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_untouched(rows_w, 0x7EEE) and guards_untouched(counts_w, -77)
    rows, counts = rows.cpu().numpy().reshape(files, cap, 4), counts.cpu().numpy()
    assert all(0 <= counts[f] <= cap and (rows[f, counts[f]:] == 0x7EEE).all() for f in range(files))
    return [rows[f, :counts[f]] for f in range(files)], counts


@pytest.mark.parametrize('files,n_in,n_frames,C_', [(1, 1, 1, 1), (3, 45, 40, 12), (2, 600, 600, 14), (5, 33, 33, 12)])
def test_decode_multi_equals_the_host_decoder(files, n_in, n_frames, C_):
    from salsa_amd.crnn.decode import decode_multi_rows, rows_to_list
    from salsa_amd.crnn.postprocess import cos_unify_of, multi_accdoa_rows
    act, xyz = ref.build_decode_inputs(files, n_in, C_, seed=files * n_in + C_)
    if files == 5:                                                 # a file with all 3 n_frames C rows (capacity full), a file with none
        act[1], xyz[1] = (a[0] for a in ref.build_decode_inputs(1, n_in, C_, seed=7, fill='all'))
        act[2], xyz[2] = (a[0] for a in ref.build_decode_inputs(1, n_in, C_, seed=8, fill='none'))
    want = [multi_accdoa_rows(act[f], xyz[f], 0.5, 15.0, C_, n_frames, eval_version='2020', as_array=True) for f in range(files)]
    got, counts = run_decode(act, xyz, n_frames, C_, 0.5, cos_unify_of(15.0))
    print('decode (%d, %d, %d, %d): %s rows' % (files, n_in, n_frames, C_, counts.tolist()))
    assert counts.tolist() == [len(w) for w in want]
    for f in range(files):
        assert np.array_equal(got[f].astype(np.int64), want[f].reshape(-1, 4)), f
    if files == 5:
        assert counts[1] == 3 * n_frames * C_ and counts[2] == 0
    if n_frames >= 33:                                             # same-class rows exist: some cell holds more than one row
        cells = got[0][:, 0].astype(np.int64) * C_ + got[0][:, 1]
        assert np.bincount(cells).max() >= 2 and (np.diff(cells) >= 0).all()
    rows_t, counts_t = decode_multi_rows(torch.from_numpy(act).to(DEV), torch.from_numpy(xyz).to(DEV), n_frames, 0.5, 15.0, C_)
    lists = rows_to_list(rows_t.cpu(), counts_t.cpu(), eval_version='2020', as_array=True)
    assert all(np.array_equal(lists[f], want[f].reshape(-1, 4)) for f in range(files))


@pytest.mark.parametrize('seed', [0, 1])
def test_decode_multi_at_the_knife_edge_of_cos_unify(seed):
    """a pair whose cosine is c0: the launch with cos_unify a few float64 ulps on either side of c0 decides as numpy does"""
    thr = np.float32(0.3)
    below = np.nextafter(thr, np.float32(0))
    vi, vj, c0 = ref.knife_edge_pair(seed)
    far = (-(vi + vj)).astype(np.float32)
    V = np.broadcast_to(np.stack([vi, vj, far]), (4, 1, 3, 3)).copy()          # (frame, class, track, axis)
    xyz = ref.from_items(V)[None]
    act = np.asarray([[thr, thr, below], [thr, thr, np.nan], [thr, below, thr], [thr, thr, thr]], np.float32)[None]
    flips = []
    for ulps in (-3, -1, 0, 1, 3):
        cu = c0
        for _ in range(abs(ulps)):
            cu = float(np.nextafter(cu, -2.0 if ulps < 0 else 2.0))
        want = ref.decode_reference(act[0], xyz[0], 4, 1, thr, cu)
        got, counts = run_decode(act, xyz, 4, 1, thr, cu)
        assert np.array_equal(got[0], want[0]), ulps
        flips.append(int(want[1][0, 0]))
    assert flips[0] == 1 and flips[-1] == 2                         # unified 3 ulps below c0, two rows 3 ulps above


def test_decode_multi_launcher_refusals_write_nothing():
    from salsa_amd import _lib
    whole, counts = guarded(2, torch.int32, -77)
    a, rows = torch.zeros(2 * 5 * 36, device=DEV), torch.zeros(2 * 3 * 5 * 4 * 4, dtype=torch.int16, device=DEV)
    for n_in, n_frames, C_, cu in ((4, 5, 4, 0.9), (5, 5, 4, float('nan')), (5, 5, 4, 1.5), (5, 0, 4, 0.9), (5, 5, 0, 0.9)):
        assert _lib.load().salsa_nn_seld_decode_multi(ptr(a), ptr(a), 2, n_in, n_frames, C_, 0.5, cu, ptr(rows), ptr(counts), stream()) == -1
    torch.cuda.synchronize()
    assert bool((whole.cpu() == -77).all())


# ---------------------------------------------------------------------------------------------------- 3. end to end
C12, N_LAB = 12, 80


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    return Trainer(DEV, total_steps=10 ** 6, output_format='multi_accdoa', n_classes=C12)


def test_fused_and_torch_losses_agree(monkeypatch):
    from salsa_amd.crnn import loss as L
    rows = 4 * N_LAB
    doa, sed, gt = ref.build_adpit_inputs(rows, C12, seed=5, prefix_only=True)
    want = ref.adpit_reference(doa, sed, gt, C12)
    s, t = (torch.from_numpy(a).to(DEV).reshape(4, N_LAB, -1) for a in (sed, gt))
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(L, 'FUSED_LOSS', fused)
        p = torch.from_numpy(doa).to(DEV).reshape(4, N_LAB, -1).requires_grad_(True)
        logit = torch.randn(4, N_LAB, 3 * C12, device=DEV, requires_grad=True)
        loss, sed_l, doa_l = L.adpit_loss({'event_frame_logit': logit, 'doa_frame_output': p}, s, t)
        assert type(loss.grad_fn).__name__.startswith('_AdpitLoss') == fused
        (loss * 1.5 + doa_l * 0.25).backward()
        assert torch.count_nonzero(logit.grad) == 0 and float(sed_l.detach()) == 0.0
        out[fused] = float(loss.detach()), p.grad.cpu().numpy().reshape(rows, -1)
    e_f, e_t = abs(out[True][0] - want['loss']), abs(out[False][0] - want['loss'])
    print('fused %.9g torch %.9g exact %.9g: err %.3g / %.3g (bounds %.3g / %.3g)' % (out[True][0], out[False][0], want['loss'], e_f, e_t,
                                                                                        ref.loss_bound(want['loss'], rows, C12),
                                                                                        ref.torch_sum_bound(want['loss'], rows, C12)))
    assert e_f <= ref.loss_bound(want['loss'], rows, C12) and e_t <= ref.torch_sum_bound(want['loss'], rows, C12)
    g = 1.75 * want['g_doa'].astype(np.float64)                     # the upstream factor is applied in float32: one more rounding
    gmax = float(np.abs(g).max())
    assert float(np.abs(out[True][1] - g).max()) <= 2.0 ** -23 * gmax and float(np.abs(out[False][1] - g).max()) <= 2.0 ** -22 * gmax


def pair_csvs(tmp_path, n_clips):
    """metadata with same-class pairs (class 3 holds tracks 0 and 1 in most frames, class 7 three tracks in some) -> (paths, rows)"""
    rng = np.random.default_rng(3)
    paths, gts = [], []
    for i in range(n_clips):
        rows = []
        for fr in range(N_LAB):
            rows.append((fr, 3, 0, int(rng.integers(-180, 180)), int(rng.integers(-40, 40))))
            if fr % 4 != i:
                rows.append((fr, 3, 1, int(rng.integers(-180, 180)), int(rng.integers(-40, 40))))
            if fr % 5 == 0:
                rows += [(fr, 7, tr, 100 * tr - 120, 10 * tr) for tr in range(3)]
            if fr % 7 == 0:
                rows.append((fr, int(rng.choice([0, 1, 2, 4, 5, 6, 8, 9, 10, 11])), 4, int(rng.integers(-180, 180)), 0))
        path = tmp_path / ('clip%d.csv' % i)
        path.write_text(''.join('%d,%d,%d,%d,%d\n' % r for r in rows))
        paths.append(str(path))
        gts.append([(r[0], r[1], r[3], r[4]) for r in rows])
    return paths, gts


def test_bf16_step_from_a_trackwise_bank_and_scored_inference(trainer, tmp_path, monkeypatch):
    from salsa_amd import augment as aug
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import DEFAULT_MARGIN, DeviceSeldScore, gt_rows_to_device
    from salsa_amd.dataset import GpuFeatureBank
    tr = trainer
    paths, gts = pair_csvs(tmp_path, 4)
    bank = GpuFeatureBank(None, n_classes=3 * C12, device=DEV, label_format='trackwise')
    feats = torch.randn(4, 7, 8 * N_LAB, 200, generator=torch.Generator().manual_seed(4)).to(DEV)
    bank.add_features(feats, ['clip%d' % i for i in range(4)], gt_meta=paths)
    bank.finalize(normalize=False)
    assert len(bank) == 4 and bank.n_dropped == 0 and float(bank.sed_all[:, 2 * C12:].sum()) > 0
    # a training batch through salsa_bank_batch: targets bit-equal to the composed path
    idx = [2, 0, 3, 1]
    draws = aug.draw_augment(4, bank.chunk_len, 200, 'foa', torch.Generator().manual_seed(6))
    draws['m'][:, :4] = torch.tensor([[1, 0, 1, 0], [0, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 1]])
    assert bank._fused()
    x, sed, doa, _ = bank.batch_augmented(idx, draws, 'foa', 'salsa')
    monkeypatch.setenv('SALSA_BANK_BATCH', '0')
    x2, sed2, doa2, _ = bank.batch_augmented(idx, draws, 'foa', 'salsa')
    monkeypatch.delenv('SALSA_BANK_BATCH')
    assert torch.equal(sed, sed2) and torch.equal(doa.view(torch.int32), doa2.view(torch.int32)) and torch.equal(x, x2)
    assert sed.shape == (4, N_LAB, 3 * C12) and doa.shape == (4, N_LAB, 9 * C12) and not torch.equal(doa, bank.batch(idx)[2])
    loss, sed_l, doa_l = (float(v) for v in tr.train_step(x, sed, doa))              # bf16 autocast, the fused ADPIT loss
    assert np.isfinite(loss) and loss > 0 and sed_l == 0.0 and doa_l == loss
    # inference: rows decoded and scored on the device against SeldMetrics on the host rows
    tape = []

    def record(xb):
        tape.append(tr.infer(xb))
        return tape[-1]
    act = tr.infer(bank.clip_batch(0, 1))[0]
    assert act.shape == (1, N_LAB, 3 * C12)
    thr = float(torch.quantile(act.flatten(), 0.8))
    kw = dict(sub_batch=2, n_label_frames=N_LAB, sed_threshold=thr, output_format='multi_accdoa', unify_deg=15.0, n_classes=C12,
              eval_version='2020')
    host = infer_pipelined(4, bank.clip_batch, record, decode='host', **kw)
    acc = DeviceSeldScore(C12, 20, 10)
    scored = infer_pipelined(4, bank.clip_batch, lambda xb, it=iter(tape): next(it), decode='device',
                             score=gt_rows_to_device(gts, DEV) + (acc,), **kw)
    assert scored == host and sum(len(r) for r in host) > 200
    cells = [(r[0], r[1]) for r in host[0]]
    assert len(set(cells)) < len(cells)                              # several rows of one class in one frame
    m = SeldMetrics(C12, 20)
    for p, g in zip(host, gts):
        m.update(p, g, max_frames=N_LAB, label_rate=10)
    print('scored: %s' % {n: getattr(m, n) for n in cases.COUNTERS})
    assert [getattr(acc, n) for n in cases.COUNTERS] == [getattr(m, n) for n in cases.COUNTERS] and m.Nref > 100 and m.DE_TP > 50
    assert abs(acc.total_DE - m.total_DE) <= max(1, m.DE_TP) * DEFAULT_MARGIN
