"""GPU tests of salsa_nn_seld_score through crnn/score.py: golden g12 and the built families of tests/seld_score_cases.py against
crnn/metrics.py::SeldMetrics, the status sets against numpy's own costs, run-to-run identity, pre-filled outputs, slack capacity with
garbage behind the counts, the distance statement, and infer_pipelined(decode='device', score=...) end to end.

Bounds.  Counters are EQUAL to SeldMetrics' after the host has scored the doubt / refused segments.  |total_DE - host| <= DE_TP x
margin: every undoubted slot average is within the measured deviation of the device's distance from numpy's, which is below
margin / 16 (profiles/seld_score_distance.txt).  A segment must be in doubt where numpy's costs put a rival pairing or a slot
average within margin / 2 and must not be where both are farther than 2 margin (the inputs hold nothing between)."""
import ctypes as C

import numpy as np
import pytest
import torch

import seld_score_cases as cases

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
    """-> (DeviceSeldScore, counters (files, n_seg, 10), total_de (files, n_seg), status (files, n_seg)) of one launch"""
    from salsa_amd.crnn.score import score_dcase_rows_async
    (pr, pc), (gr, gc) = to_device(pred_files, **pack), to_device(gt_files, **pack)
    pending = score_dcase_rows_async(pr, pc, gr, gc, margin=margin(), **kw)
    got = pending.result()
    counters, de, status = (t.cpu().numpy() for t in pending.records)
    return got, counters.reshape(status.shape + (10,)), de.reshape(status.shape), status


def check_case(name, pred_files, gt_files, kw, **pack):
    got, counters, de, status = run(pred_files, gt_files, kw, **pack)
    want_c = np.zeros(10, dtype=np.int64)
    for f, (p, g) in enumerate(zip(pred_files, gt_files)):
        for s in range(status.shape[1]):
            what = '%s: file %d segment %d' % (name, f, s)
            assert status[f, s] == cases.expected_status(p, g, s, kw, margin()), what
            ref_c, ref_de = cases.host_segment(p, g, s, kw)
            if status[f, s] == 0:
                assert list(counters[f, s]) == ref_c, what
                assert abs(de[f, s] - ref_de) <= ref_c[7] * margin(), what
            else:
                assert not counters[f, s].any() and de[f, s] == 0.0, what
            want_c += ref_c
    whole = cases.host_total(pred_files, gt_files, kw)
    assert [getattr(got, n) for n in cases.COUNTERS] == [getattr(whole, n) for n in cases.COUNTERS] == list(want_c), name
    err = abs(got.total_DE - whole.total_DE)
    print('%s: %d segments, %d doubt, %d refused, DE_TP %d, |total_DE - host| %.3g (bound %.3g)'
          % (name, status.size, got.n_doubt, got.n_refused, whole.DE_TP, err, whole.DE_TP * margin()))
    assert err <= whole.DE_TP * margin(), name
    assert (got.n_segments, got.n_doubt, got.n_refused) == (status.size, int((status == 1).sum()), int((status == 2).sum()))
    assert got.scores() == pytest.approx(whole.scores(), abs=margin()) and got.seld_error() == pytest.approx(whole.seld_error(), abs=margin())
    return got, counters, de, status


def test_g12():
    pred, gt = cases.g12_files()
    _, _, _, status = check_case('g12', pred, gt, cases.DEFAULTS)
    assert (status == 0).mean() >= 0.5 and not (status == 2).any()


FAMILIES = cases.built_families()


@pytest.mark.parametrize('k', range(len(FAMILIES)), ids=[c[0].replace(' ', '_') for c in FAMILIES])
def test_built_family(k):
    name, pred, gt, kw = FAMILIES[k]
    _, _, _, status = check_case(name, pred, gt, kw)
    assert (status == 0).mean() >= 0.5 and not (status == 2).any(), name


def test_knife_edges_go_to_the_host():
    for name, pred, gt, kw in cases.knife_edges():
        _, _, _, status = check_case(name, pred, gt, kw)
        assert list(status[:, 0]) == [1] * len(pred) and list(status[:, 1]) == [0] * len(pred), name


def test_five_doas_in_a_cell_are_refused_and_scored_on_the_host():
    rng = np.random.RandomState(5)
    pred, gt = cases.random_file(rng, max_g=2, max_p=2, density=0.3)
    five = [(13, 6, 20 * k, 5) for k in range(5)]
    files_p, files_g = [pred + five, pred, pred + [(25, 0, 0, 0)] * 7], [gt + [(13, 6, 3, 3)], gt + five, gt]
    _, _, _, status = check_case('five in a cell', files_p, files_g, dict(cases.DEFAULTS, n_frames=40))
    assert list(status[:, 1]) == [2, 2, 0] and list(status[:, 2]) == [0, 0, 2]


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
    rc = _lib.load().salsa_nn_seld_score(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], n_files, kw['n_frames'], kw['label_rate'],
                                         kw['n_classes'], float(kw['doa_threshold']), margin(), ptr(counters), ptr(de), ptr(status), ptr(sums),
                                         ptr(sum_de), C.c_void_p(stream.cuda_stream))
    assert rc == 0
    stream.synchronize()
    counters, de, status = counters.cpu().numpy(), de.cpu().numpy(), status.cpu().numpy()
    assert np.isin(status, (0, 1, 2)).all() and not np.isnan(de).any() and (counters >= 0).all()
    ok = status == 0
    assert ok.sum() >= 6 and list(sums.cpu().numpy()) == list(counters[ok].astype(np.int64).sum(axis=0))
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
    pending = score_dcase_rows_async(pr, bad, gr, gc, **kw)
    torch.cuda.synchronize()
    status = pending.records[2].cpu().numpy()
    assert (status[1] == 2).all() and not pending.records[0].cpu().numpy().reshape(status.shape + (10,))[1].any()
    with pytest.raises(ValueError, match='slab'):
        pending.result()
    with pytest.raises(ValueError, match='CUDA'):
        score_dcase_rows(pr.cpu(), pc.cpu(), gr.cpu(), gc.cpu())
    with pytest.raises(ValueError, match='refused'):
        score_dcase_rows(pr, pc, gr, gc, n_classes=33)


def test_the_distance_statement_on_the_device():
    from salsa_amd import _lib
    from salsa_amd.crnn.metrics import angular_distance_deg
    rng = np.random.RandomState(1)
    n = 20000
    q = np.stack([rng.randint(-180, 180, n), rng.randint(-90, 91, n), rng.randint(-180, 180, n), rng.randint(-90, 91, n)], axis=1).astype(np.int16)
    q[:6] = [(0, 0, 20, 0), (10, -10, 10, 10), (0, 0, 0, 0), (0, 90, 77, 90), (0, 0, 180, 0), (30, 89, 31, 89)]
    quads, out = torch.from_numpy(q).to(DEV), torch.full((n,), float('nan'), dtype=torch.float64, device=DEV)
    rc = _lib.load().salsa_nn_seld_distance(C.c_void_p(quads.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    q = q.astype(np.int64)
    err = np.abs(out.cpu().numpy() - angular_distance_deg(q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
    print('device distance: worst deviation from numpy %.3g degrees (margin / 16 = %.3g)' % (err.max(), margin() / 16))
    assert err.max() <= margin() / 16


@pytest.fixture(scope='module')
def trainer():
    from salsa_amd.crnn.train import Trainer
    torch.manual_seed(0)
    return Trainer(DEV, total_steps=10 ** 6)


def test_infer_pipelined_scores_what_the_host_scores(trainer):
    """5 clips at sub_batch 2 in 320 / 200 chunks (40 / 25 label frames of 120), the forward recorded once and replayed: the scores of
    score= against SeldMetrics on the rows decoded on the host, and the rows against a call without score="""
    from salsa_amd.crnn.infer import infer_pipelined
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import DeviceSeldScore, gt_rows_to_device
    tr = trainer
    kw = dict(sub_batch=2, depth=2, n_label_frames=120, chunk_len=320, chunk_hop_len=200, eval_version='2020')
    for seed in range(9, 17):               # (the device rounds angles in float64, the host in float32: redrawn until the ROWS agree)
        feats = torch.randn(5, 7, 960, 200, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            thr = float(torch.quantile(tr.infer(feats[:1, :, :320])[0].flatten(), 0.9))
        tape = []

        def record(x):
            tape.append(tr.infer(x))
            return tape[-1]
        host = infer_pipelined(5, lambda lo, hi: feats[lo:hi], record, sed_threshold=thr, decode='host', **kw)
        plain = infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x, it=iter(tape): next(it), sed_threshold=thr, decode='device', **kw)
        if plain == host:
            break
    assert plain == host and sum(len(r) for r in host) > 200
    rng = np.random.RandomState(seed)
    gt = [[(r[0], r[1], r[2] + int(rng.randint(-25, 26)), int(np.clip(r[3] + rng.randint(-25, 26), -90, 90))) for r in rows if rng.rand() < 0.7]
          + [(int(rng.randint(0, 120)), int(rng.randint(0, 12)), 0, 0) for _ in range(5)] for rows in host]
    acc = DeviceSeldScore()
    scored = infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x, it=iter(tape): next(it), sed_threshold=thr, decode='device',
                             score=gt_rows_to_device(gt, DEV) + (acc,), **kw)
    assert scored == plain                                                        # the rows are unchanged
    m = SeldMetrics()
    for p, g in zip(host, gt):
        m.update(p, g, max_frames=120)
    assert [getattr(acc, n) for n in cases.COUNTERS] == [getattr(m, n) for n in cases.COUNTERS] and m.DE_TP > 50
    assert abs(acc.total_DE - m.total_DE) <= m.DE_TP * margin() and acc.n_segments == 5 * 12
    assert acc.scores() == pytest.approx(m.scores(), abs=margin())
    with pytest.raises(ValueError, match="decode='device'"):
        infer_pipelined(5, lambda lo, hi: feats[lo:hi], lambda x: None, decode='host', score=gt_rows_to_device(gt, DEV) + (acc,), **kw)
