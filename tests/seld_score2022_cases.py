"""Yardsticks shared by tests/test_metrics2022_cpu.py, tests/test_seld_score2022_cpu.py and tests/test_seld_score2022_gpu.py: the inputs
of tests/seld_score_cases.py (imported, not restated) under the class-wise SELD 2022 metric -- SeldMetrics2022 per segment and over all
files -- the small built cases of the 2022 tests, and the comparison of per-segment records and of a finished result with the host.

A case is (name, pred files, gt files, kwargs) with kwargs = n_frames, label_rate, n_classes, doa_threshold, as there.  The doubt
oracle is seld_score_cases.expected_status: the 2022 metric pairs and decides exactly as the 2021 one."""
import numpy as np

import seld_score_cases as cases

FIVE = ('TP', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')                       # what the device stores per class
EIGHT = ('TP', 'FP', 'FP_spatial', 'FN', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')
DOUBT_CAP = 0.05                                                       # of the segments of a built case may go to the host


def kw_of(n_frames, label_rate=10, n_classes=12, doa_threshold=20):
    return dict(n_frames=n_frames, label_rate=label_rate, n_classes=n_classes, doa_threshold=doa_threshold)


def main_case():
    """3 files x 3 segments x 4 classes.  File 0 segment 0: class 0 ground truth only, class 1 prediction only, class 2 both without
    a common frame (two predictions at once: booked as 2 misses), class 3 a slot average under the threshold; segment 1: class 0 a
    slot average over it (FP_spatial), class 1 n_p > n_g, class 2 n_p < n_g, class 3 two DOAs of one class in a frame on both sides;
    segment 2: a plain hit.  File 1: a random mix of up to 2 x 2 cells.  File 2: empty on both sides."""
    gt0 = [(0, 0, 10, 0), (1, 0, 10, 0), (3, 2, 0, 0), (4, 3, 40, 10), (5, 3, 40, 10),
           (10, 0, 0, 0), (11, 1, 0, 0), (12, 2, 0, 0), (12, 2, 90, 0), (12, 2, -90, 30), (13, 3, 20, 0), (13, 3, -60, 10), (14, 3, 20, 0),
           (25, 0, -120, -30)]
    pred0 = [(2, 1, 30, 5), (5, 2, 0, 0), (5, 2, 90, 0), (4, 3, 45, 12), (5, 3, 43, 9),
             (10, 0, 60, 0), (11, 1, 3, 0), (11, 1, 100, 20), (11, 1, -100, -20), (12, 2, 88, 2), (13, 3, -58, 12), (13, 3, 24, 1), (14, 3, 70, 0),
             (25, 0, -118, -28)]
    pred1, gt1 = cases.random_file(np.random.RandomState(2022), n_frames=30, n_classes=4, max_g=2, max_p=2, density=0.4)
    return 'main case', [pred0, pred1, []], [gt0, gt1, []], kw_of(30, n_classes=4)


def edge_cases():
    """the edges of the class axis, of the segment grid and of the per-file reduction"""
    rng = np.random.RandomState(22)
    out = []

    def add(name, n_files, kw, **build):
        fp, fg = zip(*[cases.random_file(rng, n_frames=kw['n_frames'], n_classes=kw['n_classes'], **build) for _ in range(n_files)])
        out.append((name, list(fp), list(fg), kw))
    add('n_classes 1', 2, kw_of(30, n_classes=1), max_g=2, max_p=2, density=0.5)
    add('n_classes 32', 2, kw_of(20, n_classes=32), max_g=2, max_p=2, density=0.2)
    add('label_rate 1', 2, kw_of(12, label_rate=1, n_classes=4), max_g=2, max_p=2, density=0.5)
    add('label_rate 32', 2, kw_of(64, label_rate=32, n_classes=4), max_g=2, max_p=2, density=0.3)
    add('n_frames 25', 2, kw_of(25, n_classes=4), max_g=2, max_p=2, density=0.4)
    add('300 rows', 1, kw_of(40), max_g=2, max_p=2, density=0.8)
    add('single file', 1, kw_of(20, n_classes=3), max_g=2, max_p=2, density=0.4)
    add('33 files', 33, kw_of(20, n_classes=3), max_g=1, max_p=2, density=0.3)
    assert min(len(out[5][1][0]), len(out[5][2][0])) >= 300
    return out


def doubt_and_refusal_cases():
    """one such segment in file 1 of 3: segment 1 holds the knife edge GT (0, 0) against prediction (20, 0) at threshold 20 (doubt), or
    five predicted DOAs in one cell (refused); the other segments and files are plain"""
    rng = np.random.RandomState(7)
    files = [cases.random_file(rng, n_frames=30, n_classes=4, max_g=2, max_p=2, density=0.3, frames=[t for t in range(30) if not 10 <= t < 20])
             for _ in range(3)]
    pred, gt = [f[0] for f in files], [f[1] for f in files]
    knife_g, knife_p = [(13, 2) + cases.KNIFE_BELOW[0], (14, 1, 50, 5)], [(13, 2) + cases.KNIFE_BELOW[1], (14, 1, 52, 4)]
    five_g, five_p = [(13, 2, 3, 3), (14, 1, 50, 5)], [(13, 2, 20 * k, 5) for k in range(5)] + [(14, 1, 52, 4)]
    kw = kw_of(30, n_classes=4)
    return [('doubt in file 1', [pred[0], pred[1] + knife_p, pred[2]], [gt[0], gt[1] + knife_g, gt[2]], kw, 1),
            ('refusal in file 1', [pred[0], pred[1] + five_p, pred[2]], [gt[0], gt[1] + five_g, gt[2]], kw, 2)]


def segment_alone(rows, s, label_rate):
    return [(r[0] - s * label_rate,) + tuple(r[1:]) for r in cases.segment_rows_of(rows, s, label_rate)]


def host_segment(pred, gt, s, kw):
    """SeldMetrics2022 on segment s of one file alone, as a file of that one segment -> (five (C, 5), total_DE (C,), [S, D, I])"""
    from salsa_amd.crnn.metrics import SeldMetrics2022
    lr = kw['label_rate']
    m = SeldMetrics2022(kw['n_classes'], kw['doa_threshold'])
    m.update(segment_alone(pred, s, lr), segment_alone(gt, s, lr), max_frames=lr, label_rate=lr)
    return np.stack([getattr(m, n) for n in FIVE], axis=1), m.total_DE, [m.S, m.D, m.I]


def host_total(pred_files, gt_files, kw, average='macro'):
    """SeldMetrics2022 over all files, the way it is used: one update per file"""
    from salsa_amd.crnn.metrics import SeldMetrics2022
    m = SeldMetrics2022(kw['n_classes'], kw['doa_threshold'], average)
    for p, g in zip(pred_files, gt_files):
        m.update(p, g, max_frames=kw['n_frames'], label_rate=kw['label_rate'])
    return m


def expected_statuses(pred_files, gt_files, kw, margin):
    """(n_files, n_seg) from numpy's own costs, before anything is launched"""
    n_seg = -(-kw['n_frames'] // kw['label_rate'])
    return np.array([[cases.expected_status(p, g, s, kw, margin) for s in range(n_seg)] for p, g in zip(pred_files, gt_files)])


def check_records(name, pred_files, gt_files, kw, margin, records, de_bound):
    """the per-segment records (class counters (files, n_seg, C, 5), class total_DE (files, n_seg, C), sdi (files, n_seg, 3), status
    (files, n_seg)) against SeldMetrics2022 on every segment alone: status as numpy's costs say, integers equal, a class's total_DE
    within DE_TP[c] x de_bound, zeros where the status is not 0.  -> the sums of every file's status-0 records, added in segment order"""
    five, de, sdi, status = records
    want = expected_statuses(pred_files, gt_files, kw, margin)
    assert status.shape == want.shape and (status == want).all(), (name, status, want)
    C = kw['n_classes']
    sum_five, sum_de, sum_sdi = np.zeros((len(pred_files), C, 5), np.int64), np.zeros((len(pred_files), C)), np.zeros((len(pred_files), 3), np.int64)
    for f, (p, g) in enumerate(zip(pred_files, gt_files)):
        for s in range(status.shape[1]):
            what = '%s: file %d segment %d' % (name, f, s)
            if status[f, s] != 0:
                assert not five[f, s].any() and not sdi[f, s].any() and (de[f, s] == 0.0).all(), what
                continue
            ref5, ref_de, ref_sdi = host_segment(p, g, s, kw)
            assert (five[f, s] == ref5).all() and list(sdi[f, s]) == ref_sdi, (what, five[f, s], ref5, sdi[f, s], ref_sdi)
            assert (np.abs(de[f, s] - ref_de) <= ref5[:, 2] * de_bound).all(), (what, de[f, s], ref_de)
            sum_five[f] += five[f, s]
            sum_de[f] = sum_de[f] + de[f, s]
            sum_sdi[f] += sdi[f, s]
    return sum_five, sum_de, sum_sdi


def check_result(name, got, pred_files, gt_files, kw, margin, jackknife=True):
    """a finished DeviceSeldScore2022 against SeldMetrics2022 fed the same files: every integer counter and every file record equal,
    total_DE[c] within DE_TP[c] x margin, scores(), classwise() and (with at least 2 files) jackknife() within margin"""
    import pytest
    whole = host_total(pred_files, gt_files, kw, got.average)
    for n in EIGHT:
        assert (getattr(got, n) == getattr(whole, n)).all() and getattr(got, n).dtype == np.int64, (name, n, getattr(got, n), getattr(whole, n))
    assert (got.S, got.D, got.I) == (whole.S, whole.D, whole.I), name
    assert (got.FP == got.DE_FP).all() and (got.FN == got.DE_FN).all() and (got.FP_spatial == got.DE_TP - got.TP).all(), name
    assert (np.abs(got.total_DE - whole.total_DE) <= whole.DE_TP * margin).all(), (name, got.total_DE, whole.total_DE)
    a, b = got.file_records(), whole.file_records()
    assert sorted(a) == sorted(b) and a['TP'].shape == (len(pred_files), kw['n_classes'])
    for n in EIGHT + ('S', 'D', 'I'):
        assert (a[n] == b[n]).all(), (name, n, a[n], b[n])
    assert (np.abs(a['total_DE'] - b['total_DE']) <= b['DE_TP'] * margin).all(), name
    assert got.scores() == pytest.approx(whole.scores(), abs=margin) and got.seld_error() == pytest.approx(whole.seld_error(), abs=margin), name
    assert np.abs(got.classwise() - whole.classwise()).max() <= margin, name
    if jackknife and len(pred_files) >= 2:
        ja, jb = got.jackknife(), whole.jackknife()
        for k in jb:
            flat = lambda v: list(v[:3]) + list(v[3])                                          # noqa: E731
            assert flat(ja[k]) == pytest.approx(flat(jb[k]), abs=margin), (name, k, ja[k], jb[k])
    return whole
