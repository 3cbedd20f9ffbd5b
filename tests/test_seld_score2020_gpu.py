"""GPU tests of salsa_nn_seld_score2020 through crnn/score.py: golden g12, the built families and the knife edges of
tests/seld_score_cases.py against crnn/metrics.py::SeldMetrics2020, the status against numpy's own costs, the shapes at which the
kernel itself can go wrong, run-to-run identity, pre-filled outputs, and infer_pipelined(decode='device', score=...) end to end with
either accumulator.

Bounds.  Counters are EQUAL to SeldMetrics2020's after the host has scored the doubt / refused segments.  |total_DE - host| <= DE_TP x
margin: a class average is a mean of sums of at most four distances, each within the measured 1.207e-6 degrees of numpy's
(profiles/seld_score_distance.txt), so within margin / 20.  A segment must be in doubt where numpy's costs put a class average within
margin / 2 of the threshold and must not be where every one is farther than 2 margin (the inputs hold nothing between)."""
import ctypes as C

import numpy as np
import pytest
import torch

import seld_score_cases as cases
import seld_score2020_cases as cases20

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


def run(pred_files, gt_files, kw, **pack):
    """-> (DeviceSeldScore2020, counters (files, n_seg, 10), total_de (files, n_seg), status (files, n_seg)) of one launch"""
    from salsa_amd.crnn.score import DeviceSeldScore2020, score_dcase_rows_async
    (pr, pc), (gr, gc) = to_device(pred_files, **pack), to_device(gt_files, **pack)
    pending = score_dcase_rows_async(pr, pc, gr, gc, margin=margin(), eval_version='2020', **kw)
    got = pending.result()
    assert isinstance(got, DeviceSeldScore2020)
    counters, de, status = (t.cpu().numpy() for t in pending.records)
    return got, counters.reshape(status.shape + (10,)), de.reshape(status.shape), status


def check_case(name, pred_files, gt_files, kw, **pack):
    got, counters, de, status = run(pred_files, gt_files, kw, **pack)
    want_c = np.zeros(10, dtype=np.int64)
    for f, (p, g) in enumerate(zip(pred_files, gt_files)):
        for s in range(status.shape[1]):
            what = '%s: file %d segment %d' % (name, f, s)
            assert status[f, s] == cases20.expected_status(p, g, s, kw, margin()), what
            ref_c, ref_de = cases20.host_segment(p, g, s, kw)
            if status[f, s] == 0:
                assert list(counters[f, s]) == ref_c, what
                assert abs(de[f, s] - ref_de) <= ref_c[cases20.DE_TP] * margin(), what
            else:
                assert not counters[f, s].any() and de[f, s] == 0.0, what
            want_c += ref_c
    whole = cases20.host_total(pred_files, gt_files, kw)
    assert [getattr(got, n) for n in cases20.COUNTERS] == [getattr(whole, n) for n in cases20.COUNTERS] == list(want_c), name
    err = abs(got.total_DE - whole.total_DE)
    print('%s: %d segments, %d doubt, %d refused, DE_TP %d, |total_DE - host| %.3g (bound %.3g)'
          % (name, status.size, got.n_doubt, got.n_refused, whole.DE_TP, err, whole.DE_TP * margin()))
    assert err <= whole.DE_TP * margin(), name
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    if whole.Nref:
        assert got.scores() == pytest.approx(whole.scores(), abs=margin()) and got.seld_error() == pytest.approx(whole.seld_error(), abs=margin())
    return got, counters, de, status


def test_g12():
    pred, gt = cases.g12_files()
    got, _, _, status = check_case('g12', pred, gt, cases.DEFAULTS)
    assert not status.any() and (got.TP, got.Nref, got.Nsys, got.DE_TP) == (113, 290, 219, 182)        # the reference's own (golden g29)


FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(k):
    """(among them: n_frames 45 at rate 10, a short last segment; n_classes 14 with rows of classes 14 and 15 present; shuffled rows)"""
    name, pred, gt, kw = FAMILIES[k]
    _, _, _, status = check_case(name, pred, gt, kw)
    assert not status.any(), name


def test_knife_edges_go_to_the_host_and_rival_maps_do_not():
    for name, pred, gt, kw in cases.knife_edges():
        _, _, _, status = check_case(name, pred, gt, kw)
        assert list(status[:, 0]) == [1, 1, 0, 0, 0, 0] and not status[:, 1].any(), name


def test_five_doas_in_a_cell_are_refused_and_scored_on_the_host():
    name, files_p, files_g, kw = cases20.five_in_a_cell()
    _, _, _, status = check_case(name, files_p, files_g, kw)
    assert list(status[:, 1]) == [2, 2, 0] and list(status[:, 2]) == [0, 0, 2] and not (status == 1).any()


def test_more_rows_than_one_tile_and_the_largest_cell_grid():
    """600 rows a side (more than two tiles of 256) in shuffled order at 32 classes x label rate 32: every LDS cell index is used"""
    rng = np.random.RandomState(32)
    kw = dict(n_frames=64, label_rate=32, n_classes=32, doa_threshold=20)
    files = [cases.random_file(rng, n_frames=64, n_classes=32, max_g=2, max_p=2, density=0.45) for _ in range(3)]
    shuffle = lambda rows: [rows[i] for i in rng.permutation(len(rows))]          # noqa: E731
    pred, gt = [shuffle(f[0]) for f in files], [shuffle(f[1]) for f in files]
    assert min(len(r) for r in pred + gt) > 600
    check_case('32 x 32 cells', pred, gt, kw)


def test_two_launches_are_bit_identical_and_slack_capacity_changes_nothing():
    name, pred, gt, kw = next(c for c in FAMILIES if c[0] == 'shuffled rows')
    a, b = run(pred, gt, kw), run(pred, gt, kw)
    c = run(pred, gt, kw, slack=300, garbage=(3, 2, 17, 5))                        # rows of a real segment and class behind the counts
    assert a[0].DE_TP > 10
    for u, v, w in zip(a[1:], b[1:], c[1:]):
        assert u.tobytes() == v.tobytes() == w.tobytes()
    assert a[0].total_DE == b[0].total_DE == c[0].total_DE and a[0].TP == c[0].TP


def test_every_output_is_overwritten_and_the_sums_are_the_records():
    from salsa_amd import _lib
    name, pred, gt, kw = next(c for c in FAMILIES if c[0] == 'up to 4 x 4')
    (pr, pc), (gr, gc) = to_device(pred), to_device(gt)
    n_files, n_seg = len(pred), 4
    counters = torch.full((n_files * n_seg, 10), SENTINEL, dtype=torch.int32, device=DEV)
    de = torch.full((n_files * n_seg,), float('nan'), dtype=torch.float64, device=DEV)
    status = torch.full((n_files * n_seg,), SENTINEL, dtype=torch.int32, device=DEV)
    sums = torch.full((10,), SENTINEL, dtype=torch.int64, device=DEV)
    sum_de = torch.full((1,), float('nan'), dtype=torch.float64, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    rc = _lib.load().salsa_nn_seld_score2020(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], n_files, kw['n_frames'],
                                             kw['label_rate'], kw['n_classes'], float(kw['doa_threshold']), margin(), ptr(counters), ptr(de),
                                             ptr(status), ptr(sums), ptr(sum_de), C.c_void_p(stream.cuda_stream))
    assert rc == 0
    stream.synchronize()
    counters, de, status = counters.cpu().numpy(), de.cpu().numpy(), status.cpu().numpy()
    assert np.isin(status, (0, 1, 2)).all() and not np.isnan(de).any() and (counters >= 0).all()
    ok = status == 0
    assert ok.sum() >= 6 and list(sums.cpu().numpy()) == list(counters[ok].astype(np.int64).sum(axis=0))
    assert (counters[ok][:, [0, 1, 2, 3]].sum(axis=1) == kw['n_classes']).all()   # TP + FP + FN + TN: every class of a segment is one of them
    total = 0.0
    for v in de[ok]:
        total += float(v)
    assert float(sum_de.cpu()[0]) == total                                        # one running sum in record order


def test_a_count_above_the_capacity_reads_nothing_and_is_an_error():
    from salsa_amd.crnn.score import score_dcase_rows, score_dcase_rows_async
    name, pred, gt, kw = FAMILIES[0]
    (pr, pc), (gr, gc) = to_device(pred), to_device(gt)
    bad = pc.clone()
    bad[1] = pr.shape[1] + 1
    pending = score_dcase_rows_async(pr, bad, gr, gc, eval_version='2020', **kw)
    torch.cuda.synchronize()
    status = pending.records[2].cpu().numpy()
    assert (status[1] == 2).all() and not pending.records[0].cpu().numpy().reshape(status.shape + (10,))[1].any()
    with pytest.raises(ValueError, match='slab'):
        pending.result()
    with pytest.raises(ValueError, match='salsa_nn_seld_score2020 refused'):
        score_dcase_rows(pr, pc, gr, gc, n_classes=33, eval_version='2020')
    with pytest.raises(ValueError, match='Unknown eval_version'):
        score_dcase_rows(pr, pc, gr, gc, eval_version='2019')


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    return Trainer(DEV, total_steps=10 ** 6)


def test_infer_pipelined_scores_by_the_type_of_the_accumulator(trainer):
    """5 clips at sub_batch 2 in 320 / 200 chunks (40 / 25 label frames of 120), the forward recorded once and replayed, rows in the 2020
    form: a DeviceSeldScore2020(n_classes=14) accumulator gives SeldMetrics2020's scores of the returned rows, a DeviceSeldScore one
    with the same eval_version='2020' still gives SeldMetrics'"""
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics, SeldMetrics2020
    from salsa_amd.crnn.score import DeviceSeldScore, DeviceSeldScore2020, gt_rows_to_device
    tr = trainer
    kw = dict(sub_batch=2, depth=2, n_label_frames=120, chunk_len=320, chunk_hop_len=200, eval_version='2020', decode='device')
    feats = torch.randn(5, 7, 960, 200, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        thr = float(torch.quantile(tr.infer(feats[:1, :, :320])[0].flatten(), 0.9))
    tape = []

    def record(x):
        tape.append(tr.infer(x))
        return tape[-1]
    plain = infer_pipelined(5, lambda lo, hi: feats[lo:hi], record, sed_threshold=thr, **kw)
    assert sum(len(r) for r in plain) > 200 and all(len(r) == 4 for rows in plain for r in rows)
    rng = np.random.RandomState(9)
    gt = [[(r[0], r[1], r[2] + int(rng.randint(-25, 26)), int(np.clip(r[3] + rng.randint(-25, 26), -90, 90))) for r in rows if rng.rand() < 0.7]
          + [(int(rng.randint(0, 120)), int(rng.randint(0, 14)), 0, 0) for _ in range(5)] for rows in plain]
    for acc, host, names in ((DeviceSeldScore2020(n_classes=14), SeldMetrics2020(14), cases20.COUNTERS),
                             (DeviceSeldScore(), SeldMetrics(), cases.COUNTERS)):
        scored = infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x, it=iter(tape): next(it), sed_threshold=thr,
                                 score=gt_rows_to_device(gt, DEV) + (acc,), **kw)
        assert scored == plain                                                    # the rows are unchanged
        for p, g in zip(scored, gt):
            host.update(p, g, max_frames=120)
        assert [getattr(acc, n) for n in names] == [getattr(host, n) for n in names] and host.DE_TP > 30, type(acc).__name__
        assert abs(acc.total_DE - host.total_DE) <= host.DE_TP * margin() and acc.n_segments == 5 * 12
        assert acc.scores() == pytest.approx(host.scores(), abs=margin())
    assert not hasattr(acc, 'Nsys') and acc.DE_FN >= 0                            # (the second one: the 2021 counters)
