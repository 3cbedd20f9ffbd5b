"""GPU tests of salsa_nn_seld_score2022 through crnn/score.py: the main case, the edges of the class axis and of the per-file
reduction, the built families and knife edges of tests/seld_score_cases.py against crnn/metrics.py::SeldMetrics2022; doubt and refusal
resolved into the right file; pre-filled outputs, slack capacity, run-to-run identity; the 2021 and 2020 exports unchanged by a 2022
call; infer_pipelined(score=...), validate and Trainer.fit with eval_version='2022' end to end.

Bounds.  Per (file, segment): the class counters, S, D, I and the status are EQUAL to SeldMetrics2022 on the segment alone, a class's
total_DE within DE_TP[c] x margin (a slot average is a mean of distances each within the measured 1.207e-6 degrees of numpy's,
profiles/seld_score_distance.txt; margin is 83 times that).  The per-file sums are EQUAL to that file's status-0 records added in
segment order, float64 included.  After result(): every integer counter and every file record equal to the host's, total_DE[c] within
DE_TP[c] x margin, scores(), classwise() and jackknife() within margin.  At most 5 % of a built case's segments may be doubt or
refused by numpy's own costs (asserted before the launch), so the device path is what is tested."""
import ctypes as C

import numpy as np
import pytest
import torch

import seld_score_cases as cases
import seld_score2022_cases as cases22

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = -7


def margin():
    from salsa_amd.crnn.score import DEFAULT_MARGIN
    return DEFAULT_MARGIN


def to_device(files, slack=0, garbage=None):
    """row lists -> (rows, counts) on the device; slack more rows of capacity, filled with `garbage` rows behind the counts"""
    from salsa_amd.crnn.score import pack_rows
    rows, counts = pack_rows(files)
    if slack:
        rows = np.concatenate([rows, np.zeros((rows.shape[0], slack, 4), dtype=np.int16)], axis=1)
    if garbage is not None:
        for f in range(rows.shape[0]):
            rows[f, counts[f]:] = garbage
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(counts).to(DEV)


def run(pred_files, gt_files, kw, average='macro', **pack):
    """-> (DeviceSeldScore2022, (class counters (files, n_seg, C, 5), class total_DE (files, n_seg, C), sdi (files, n_seg, 3), status
    (files, n_seg)), (file counters, file total_DE, file sdi)) of one launch"""
    from salsa_amd.crnn.score import DeviceSeldScore2022, score_dcase_rows_async
    (pr, pc), (gr, gc) = to_device(pred_files, **pack), to_device(gt_files, **pack)
    pending = score_dcase_rows_async(pr, pc, gr, gc, margin=margin(), eval_version='2022', average=average, **kw)
    got = pending.result()
    assert isinstance(got, DeviceSeldScore2022) and got.average == average
    five, de, sdi, status = (t.cpu().numpy() for t in pending.records)
    n, n_seg, nc = status.shape + (kw['n_classes'],)
    sums = (pending.host['sums'].numpy().copy(), pending.host['sum_de'].numpy().copy(), pending.host['sum_sdi'].numpy().copy())
    return got, (five.reshape(n, n_seg, nc, 5), de.reshape(n, n_seg, nc), sdi.reshape(n, n_seg, 3), status), sums


def check_case(name, pred_files, gt_files, kw, average='macro', cap=True, **pack):
    want = cases22.expected_statuses(pred_files, gt_files, kw, margin())                   # on the CPU, before the launch
    if cap:
        assert (want != 0).mean() <= cases22.DOUBT_CAP, name
    got, records, sums = run(pred_files, gt_files, kw, average, **pack)
    want_sums = cases22.check_records(name, pred_files, gt_files, kw, margin(), records, margin())
    want_de = np.zeros_like(sums[1])                                                       # the device's own records in segment order
    for f in range(want_de.shape[0]):
        for s in np.nonzero(records[3][f] == 0)[0]:
            want_de[f] = want_de[f] + records[1][f, s]
    assert (sums[0] == want_sums[0]).all() and (sums[2] == want_sums[2]).all() and sums[1].tobytes() == want_de.tobytes(), name
    status = records[3]
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    whole = cases22.check_result(name, got, pred_files, gt_files, kw, margin())
    print('%s: %d segments, %d doubt, %d refused, DE_TP %d, max |total_DE[c] - host| %.3g'
          % (name, status.size, got.n_doubt, got.n_refused, whole.DE_TP.sum(), np.abs(got.total_DE - whole.total_DE).max()))
    return got, records, sums


SMALL = [cases22.main_case()] + cases22.edge_cases()


@pytest.mark.parametrize('k', range(len(SMALL)), ids=[c[0].replace(' ', '_') for c in SMALL])
def test_main_case_and_edges(k):
    """(the main case; n_classes 1 and 32; label_rate 1 and 32; a short last segment; 300 rows in one file, across the 256-row tile; a
    single file; 33 files)"""
    name, pred, gt, kw = SMALL[k]
    got, records, _ = check_case(name, pred, gt, kw, average='micro' if k % 2 else 'macro')
    if name == 'main case':
        f0 = {n: v[0] for n, v in got.file_records().items()}                              # file 0, by hand (main_case's docstring)
        assert [list(f0[n]) for n in ('TP', 'FP', 'FP_spatial', 'FN', 'Nref')] == [[1, 1, 1, 2], [0, 3, 0, 0], [1, 0, 0, 1], [1, 0, 4, 0], [3, 1, 4, 3]]
        assert (f0['S'], f0['D'], f0['I']) == (3, 2, 2) and not records[3].any() and not any(v[2].any() for v in got.file_records().values())


FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(k):
    name, pred, gt, kw = FAMILIES[k]
    check_case(name, pred, gt, kw)


def test_g12_and_the_knife_edges():
    pred, gt = cases.g12_files()
    got, records, _ = check_case('g12', pred, gt, cases.DEFAULTS)
    old = cases.host_total(pred, gt, cases.DEFAULTS)
    assert not records[3].any() and (int(got.TP.sum()), int(got.Nref.sum()), int(got.DE_TP.sum())) == (old.TP, old.Nref, old.DE_TP)
    for name, pred, gt, kw in cases.knife_edges():
        _, records, _ = check_case(name, pred, gt, kw, cap=False)                          # (built to be in doubt)
        assert records[3][:, 0].all() and not records[3][:, 1].any(), name


@pytest.mark.parametrize('k', range(2), ids=['doubt', 'refusal'])
def test_a_doubt_or_refused_segment_comes_back_empty_and_is_resolved_into_its_own_file(k):
    name, pred, gt, kw, want = cases22.doubt_and_refusal_cases()[k]
    got, records, sums = check_case(name, pred, gt, kw, cap=False)
    five, de, sdi, status = records
    assert status[1, 1] == want and (np.delete(status.reshape(-1), 4) == 0).all()
    assert not five[1, 1].any() and not sdi[1, 1].any() and not de[1, 1].any()
    alone = cases22.host_segment(pred[1], gt[1], 1, kw)
    assert alone[0][:, 1].sum() > 0
    rec = got.file_records()                                                               # (check_result held them to the host's, file by file)
    assert (rec['Nref'][1] == sums[0][1, :, 1] + alone[0][:, 1]).all() and (rec['Nref'][[0, 2]] == sums[0][[0, 2], :, 1]).all()


def raw_outputs(n_files, n_seg, nc):
    return (torch.full((n_files * n_seg, nc, 5), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((n_files * n_seg, nc), float('nan'), dtype=torch.float64, device=DEV),
            torch.full((n_files * n_seg, 3), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((n_files * n_seg,), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((n_files, nc, 5), SENTINEL, dtype=torch.int64, device=DEV),
            torch.full((n_files, nc), float('nan'), dtype=torch.float64, device=DEV),
            torch.full((n_files, 3), SENTINEL, dtype=torch.int64, device=DEV))


def test_every_output_is_overwritten_slack_changes_nothing_and_two_launches_are_bit_identical():
    from salsa_amd import _lib
    name, pred, gt, kw = next(c for c in FAMILIES if c[0] == 'shuffled rows')
    n_files, n_seg, nc = len(pred), 4, kw['n_classes']
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    stream = torch.cuda.Stream(DEV)
    results = []
    for pack in ({}, {}, dict(slack=300, garbage=(3, 2, 17, 5))):                 # rows of a real segment and class behind the counts
        (pr, pc), (gr, gc) = to_device(pred, **pack), to_device(gt, **pack)
        outs = raw_outputs(n_files, n_seg, nc)
        torch.cuda.synchronize()
        rc = _lib.load().salsa_nn_seld_score2022(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], n_files, kw['n_frames'],
                                                 kw['label_rate'], nc, float(kw['doa_threshold']), margin(), *[ptr(t) for t in outs],
                                                 C.c_void_p(stream.cuda_stream))
        assert rc == 0
        stream.synchronize()
        results.append([t.cpu().numpy() for t in outs])
    five, de, sdi, status, f_five, f_de, f_sdi = results[0]
    assert np.isin(status, (0, 1, 2)).all() and (five >= 0).all() and (sdi >= 0).all() and (f_five >= 0).all() and (f_sdi >= 0).all()
    assert not np.isnan(de).any() and not np.isnan(f_de).any() and f_five[:, :, 2].sum() > 10
    for a, b, c in zip(*results):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    # the per-record outputs alone (no file sums): the same records
    (pr, pc), (gr, gc) = to_device(pred), to_device(gt)
    outs = raw_outputs(n_files, n_seg, nc)
    rc = _lib.load().salsa_nn_seld_score2022(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], n_files, kw['n_frames'], kw['label_rate'],
                                             nc, float(kw['doa_threshold']), margin(), *[ptr(t) for t in outs[:4]], None, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and all(t.cpu().numpy().tobytes() == r.tobytes() for t, r in zip(outs[:4], results[0][:4]))


def test_a_count_above_the_capacity_reads_nothing_and_is_an_error():
    from salsa_amd.crnn.score import score_dcase_rows, score_dcase_rows_async
    name, pred, gt, kw = cases22.main_case()
    (pr, pc), (gr, gc) = to_device(pred), to_device(gt)
    bad = pc.clone()
    bad[1] = pr.shape[1] + 1
    pending = score_dcase_rows_async(pr, bad, gr, gc, eval_version='2022', **kw)
    torch.cuda.synchronize()
    five, de, sdi, status = (t.cpu().numpy() for t in pending.records)
    assert (status[1] == 2).all() and not status[[0, 2]].any()
    assert not five.reshape(3, 3, 4, 5)[1].any() and not de.reshape(3, 3, 4)[1].any() and not sdi.reshape(3, 3, 3)[1].any()
    assert not pending.host['sums'][1].any() and pending.host['sums'][0].any()
    with pytest.raises(ValueError, match='slab'):
        pending.result()
    with pytest.raises(ValueError, match='salsa_nn_seld_score2022 refused'):
        score_dcase_rows(pr, pc, gr, gc, n_classes=33, eval_version='2022')
    with pytest.raises(ValueError, match='Unknown eval_version'):
        score_dcase_rows(pr, pc, gr, gc, eval_version='2019')


def test_the_2021_and_2020_exports_are_unchanged_by_a_2022_call():
    from salsa_amd.crnn.score import score_dcase_rows_async
    name, pred, gt, kw = next(c for c in FAMILIES if c[0] == 'up to 4 x 4')
    (pr, pc), (gr, gc) = to_device(pred), to_device(gt)

    def records(version):
        pending = score_dcase_rows_async(pr, pc, gr, gc, margin=margin(), eval_version=version, **kw)
        got = pending.result()
        return [t.cpu().numpy().tobytes() for t in pending.records] + [pending.host['sums'].numpy().tobytes(), pending.host['sum_de'].numpy().tobytes()], got
    before = {v: records(v) for v in ('2021', '2020')}
    assert records('2022')[1].DE_TP.sum() > 10
    after = {v: records(v) for v in ('2021', '2020')}
    for v in before:
        assert before[v][0] == after[v][0], v
    old = cases.host_total(pred, gt, kw)
    assert [getattr(after['2021'][1], n) for n in cases.COUNTERS] == [getattr(old, n) for n in cases.COUNTERS]


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    return Trainer(DEV, total_steps=10 ** 6, n_classes=4)


def test_infer_pipelined_scores_by_the_type_of_the_accumulator(trainer):
    """4 clips at sub_batch 3 (two sub-batches, merged in order): a DeviceSeldScore2022(4) accumulator gives SeldMetrics2022's counters,
    file records and jackknife of the rows the same call returns; a DeviceSeldScore one still scores 2021"""
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import DeviceSeldScore, DeviceSeldScore2022, gt_rows_to_device
    tr = trainer
    kw = dict(sub_batch=3, depth=2, n_label_frames=40, eval_version='2020', decode='device', n_classes=4)
    feats = torch.randn(4, 7, 320, 200, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        thr = float(torch.quantile(tr.infer(feats[:1])[0].flatten(), 0.4))      # (a fresh model: whole classes lie above or below)
    tape = []

    def record(x):
        tape.append(tr.infer(x))
        return tape[-1]
    plain = infer_pipelined(4, lambda lo, hi: feats[lo:hi], record, sed_threshold=thr, **kw)
    assert sum(len(r) for r in plain) > 60 and all(len(r) == 4 for rows in plain for r in rows)
    rng = np.random.RandomState(9)
    gt = [[(r[0], r[1], r[2] + int(rng.randint(-25, 26)), int(np.clip(r[3] + rng.randint(-25, 26), -90, 90))) for r in rows if rng.rand() < 0.7]
          + [(int(rng.randint(0, 40)), int(rng.randint(0, 4)), 0, 0) for _ in range(5)] for rows in plain]
    case_kw = cases22.kw_of(40, n_classes=4)
    for acc in (DeviceSeldScore2022(4), DeviceSeldScore2022(4, average='micro'), DeviceSeldScore(4)):
        scored = infer_pipelined(4, lambda lo, hi: feats[lo:hi], lambda x, it=iter(tape): next(it), sed_threshold=thr,
                                 score=gt_rows_to_device(gt, DEV) + (acc,), **kw)
        assert scored == plain and acc.n_segments == 4 * 4                         # the rows are unchanged
        if isinstance(acc, DeviceSeldScore2022):
            whole = cases22.check_result(acc.average, acc, scored, gt, case_kw, margin())
            assert whole.DE_TP.sum() > 20 and (whole.DE_TP > 0).sum() >= 2 and acc.file_records()['TP'].shape == (4, 4)
        else:
            host = SeldMetrics(4)
            for p, g in zip(scored, gt):
                host.update(p, g, max_frames=40)
            assert [getattr(acc, n) for n in cases.COUNTERS] == [getattr(host, n) for n in cases.COUNTERS] and not hasattr(acc, 'FP_spatial')


def test_validate_and_fit_select_by_the_macro_score(tmp_path):
    """2 validation clips of 256 frames (32 label frames) from feature files: validate(eval_version='2022') on the device equals
    SeldMetrics2022 on the rows the same call returns; one epoch of Trainer.fit records that macro valSeld and names the best
    checkpoint by it; '2021' still gives the pooled figure"""
    import os
    from salsa_amd import io as sio
    from salsa_amd.crnn.fit import best_name, validate
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    frames, nf, nc = 256, 200, 12
    g = torch.Generator().manual_seed(3)
    files = [sio.save_arrays(str(tmp_path / ('clip%d.h5' % i)), feature=torch.randn(7, frames, nf, generator=g).numpy()) for i in range(2)]
    sed = (torch.rand(2, frames // 8, nc, generator=g) < 0.2).float()
    v = torch.randn(2, frames // 8, 3, nc, generator=g)
    doa = ((v / v.norm(dim=2, keepdim=True)) * sed[:, :, None, :]).reshape(2, frames // 8, 3 * nc)
    bank = GpuFeatureBank(None, chunk_len_s=128 / 80, chunk_hop_len_s=128 / 80, n_classes=nc, device='cuda')
    bank.set_scaler(np.zeros((4, 1, nf), np.float32), np.ones((4, 1, nf), np.float32))
    bank.add_feature_files(files, sed=sed.numpy(), doa=doa.numpy())
    bank = bank.finalize()
    rng = np.random.RandomState(4)
    gt = [[(f, int(rng.randint(nc)), int(rng.randint(-180, 180)), int(rng.randint(-40, 40)), 0) for f in range(0, frames // 8, 2)] for _ in range(2)]
    tr = Trainer('cuda', seed=11)
    val = validate(tr, bank, gt, eval_version='2022', return_rows=True)
    assert sum(len(r) for r in val['rows']) > 0 and val['scorer'].eval_version == '2022' and val['scorer'].average == 'macro'
    whole = cases22.check_result('validate', val['scorer'], val['rows'], gt, cases22.kw_of(frames // 8, bank.label_rate, nc), margin())
    assert (val['valER'], val['valF1'], val['valLR']) == whole.scores()[:2] + whole.scores()[3:]
    assert abs(val['valLE'] - whole.scores()[2]) <= margin() and abs(val['valSeld'] - whole.seld_error()) <= margin()
    pooled = validate(tr, bank, gt, eval_version='2021')
    assert pooled['valER'] == val['valER'] and pooled['valSeld'] != val['valSeld'] and not hasattr(pooled['scorer'], 'FP_spatial')
    hist = tr.fit(bank, val_bank=bank, val_gt=gt, batch_size=4, max_epochs=1, audio_format='mic', eval_version='2022', out_dir=str(tmp_path / 'run'))
    after = validate(tr, bank, gt, eval_version='2022')
    assert hist['best']['valSeld'] == after['valSeld'] == float(after['scorer'].seld_error())
    assert os.listdir(str(tmp_path / 'run' / 'best')) == [best_name(0, hist['best'])]
    with pytest.raises(ValueError, match='Unknown eval_version'):
        tr.fit(bank, val_bank=bank, val_gt=gt, max_epochs=1, eval_version='2023')
