"""Yardsticks shared by tests/test_seld_score2020_cpu.py and tests/test_seld_score2020_gpu.py: the inputs of tests/seld_score_cases.py
(imported, not restated) under the SELD 2020 metric -- SeldMetrics2020 per segment and the 2020 doubt oracle from numpy's own costs.

A case is (name, pred files, gt files, kwargs) with kwargs = n_frames, label_rate, n_classes, doa_threshold, as there."""
import itertools

import numpy as np

import seld_score_cases as cases

COUNTERS = ('TP', 'FP', 'FN', 'TN', 'S', 'D', 'I', 'Nref', 'Nsys', 'DE_TP')
DE_TP = COUNTERS.index('DE_TP')
# degrees per distance: four times the 7.2e-13 by which numpy's arccos differs from the C library's where numpy dispatches to its own
# loops (measured; tests/test_seld_score_cpu.py), rounded up as NUMPY_ACOS_DEG there -- a class average is a mean of sums of at most
# four distances
NUMPY_ACOS_DEG4 = 4e-12


def five_in_a_cell():
    """the one input with a refused cell: five DOAs in cell (frame 13, class 6) of the prediction, of the ground truth, and seven
    equal predictions in (25, 0)"""
    rng = np.random.RandomState(5)
    pred, gt = cases.random_file(rng, max_g=2, max_p=2, density=0.3)
    five = [(13, 6, 20 * k, 5) for k in range(5)]
    return ('five in a cell', [pred + five, pred, pred + [(25, 0, 0, 0)] * 7], [gt + [(13, 6, 3, 3)], gt + five, gt],
            dict(cases.DEFAULTS, n_frames=40))


def host_segment(pred, gt, s, kw, metrics_cls=None):
    """SeldMetrics2020 on segment s of one file alone, as a file of that one segment (every class of an EMPTY segment is a true
    negative in this metric, so a file of full length would add the other segments' again) -> (ten counters, total_DE)"""
    from salsa_amd.crnn.metrics import SeldMetrics2020
    lr = kw['label_rate']
    m = (metrics_cls or SeldMetrics2020)(kw['n_classes'], kw['doa_threshold'])
    m.update(*([(r[0] - s * lr,) + tuple(r[1:]) for r in cases.segment_rows_of(rows, s, lr)] for rows in (pred, gt)), max_frames=lr, label_rate=lr)
    return [getattr(m, n) for n in COUNTERS], m.total_DE


def host_total(pred_files, gt_files, kw):
    """SeldMetrics2020 over all files, the way it is used"""
    from salsa_amd.crnn.metrics import SeldMetrics2020
    m = SeldMetrics2020(kw['n_classes'], kw['doa_threshold'])
    for p, g in zip(pred_files, gt_files):
        m.update(p, g, max_frames=kw['n_frames'], label_rate=kw['label_rate'])
    return m


def segment_clearance(pred, gt, s, kw):
    """numpy's own view of segment s -> (smallest gap between the best and another map's total cost over its common frames, smallest
    |class average - threshold|), inf where there is none; None when a cell holds more than 4.  Only the second makes doubt in the
    2020 metric; the first says where scipy's choice among near-ties may round the minimum differently from the brute force."""
    from salsa_amd.crnn.metrics import angular_distance_deg, segment_rows
    lr = kw['label_rate']
    ps, gs = (segment_rows(cases.segment_rows_of(r, s, lr), kw['n_frames'], lr)[s] for r in (pred, gt))
    gap, edge = np.inf, np.inf
    for c in range(kw['n_classes']):
        g, p = gs.get(c), ps.get(c)
        if any(len(v) > 4 for side in (g, p) if side for v in side.values()):
            return None
        if not (g and p):
            continue
        total, n = 0.0, 0
        for frame in sorted(g):
            if frame not in p:
                continue
            ga, pa = np.array(g[frame], dtype=np.float64), np.array(p[frame], dtype=np.float64)
            cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
            n_g, n_p = cost.shape
            if n_g <= n_p:
                totals = sorted(sum(cost[i, m[i]] for i in range(n_g)) for m in itertools.permutations(range(n_p), n_g))
            else:
                totals = sorted(sum(cost[m[i], i] for i in range(n_p)) for m in itertools.permutations(range(n_g), n_p))
            if len(totals) > 1:
                gap = min(gap, totals[1] - totals[0])
            total += totals[0]
            n += 1
        if n:
            edge = min(edge, abs(total / n - kw['doa_threshold']))
    return gap, edge


def expected_status(pred, gt, s, kw, margin):
    """2 for a cell of more than 4; 1 where numpy's costs put a class average within margin / 2 of the threshold; 0 where every one
    is farther than 2 margin; the inputs are built so that nothing lies between (asserted here)"""
    cl = segment_clearance(pred, gt, s, kw)
    if cl is None:
        return 2
    assert cl[1] < margin / 2 or cl[1] > 2 * margin, 'segment %d lies between margin / 2 and 2 margin (%r): rebuild the input' % (s, cl)
    return 1 if cl[1] < margin / 2 else 0
