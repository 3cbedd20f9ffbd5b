"""Inputs and yardsticks shared by tests/test_seld_score_cpu.py and tests/test_seld_score_gpu.py: the g12 file pairs as row lists,
the built families, SeldMetrics per segment, and the doubt oracle from numpy's own costs.

Rows are (frame, class, azimuth, elevation) integers.  A case is (name, pred files, gt files, kwargs) with kwargs = n_frames,
label_rate, n_classes, doa_threshold."""
import itertools

import numpy as np

from conftest import load_golden

COUNTERS = ('TP', 'FP', 'FN', 'S', 'D', 'I', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')
DEFAULTS = dict(n_frames=600, label_rate=10, n_classes=12, doa_threshold=20)
KNIFE_BELOW, KNIFE_ABOVE = ((0, 0), (20, 0)), ((10, -10), (10, 10))      # 19.999999999999993 and 20.00000000000001 degrees


def g12_files():
    """-> (pred files, gt files) of golden g12 (columns frame, class, track, azimuth, elevation)"""
    meta, a = load_golden('g12_metrics')
    pick = lambda rows: [(int(r[0]), int(r[1]), int(r[3]), int(r[4])) for r in rows]          # noqa: E731
    return [pick(a['pred%d' % f]) for f in range(meta['n_files'])], [pick(a['gt%d' % f]) for f in range(meta['n_files'])]


def random_file(rng, n_frames=40, n_classes=12, max_g=1, max_p=1, density=0.15, spread=30, frames=None):
    """one file pair: per (frame, class) with probability `density` 0 .. max_g reference DOAs and 0 .. max_p predicted DOAs, the
    predicted ones within `spread` degrees (per angle) of reference ones so that hits and misses both occur"""
    pred, gt = [], []
    for t in (range(n_frames) if frames is None else frames):
        for c in range(n_classes):
            if rng.rand() >= density:
                continue
            n_g, n_p = rng.randint(0, max_g + 1), rng.randint(0, max_p + 1)
            doas = [(int(rng.randint(-180, 180)), int(rng.randint(-60, 61))) for _ in range(max(n_g, n_p))]
            gt += [(t, c) + d for d in doas[:n_g]]
            for azi, ele in [doas[i] for i in rng.permutation(len(doas))[:n_p]]:
                a = (azi + int(rng.randint(-spread, spread + 1)) + 180) % 360 - 180
                pred.append((t, c, a, int(np.clip(ele + rng.randint(-spread, spread + 1), -90, 90))))
    return pred, gt


def fixed_cells(rng, n_g, n_p, n_frames=30, n_classes=12):
    """cells of exactly n_g reference and n_p predicted DOAs (classes 2 and 7, every third frame), directions far apart"""
    pred, gt = [], []
    for t in range(0, n_frames, 3):
        for c in (2, 7):
            base = rng.permutation(8)[:max(n_g, n_p)]
            doas = [(int(-170 + 43 * b + rng.randint(-5, 6)), int(rng.randint(-40, 41))) for b in base]
            gt += [(t, c) + d for d in doas[:n_g]]
            pred += [(t, c, d[0] + int(rng.randint(-25, 26)), d[1] + int(rng.randint(-25, 26))) for d in reversed(doas[-n_p:])]
    return pred, gt


def built_families():
    """-> list of (name, pred files, gt files, kwargs): 3 to 6 files of 60 frames or fewer each"""
    rng = np.random.RandomState(2021)
    small = dict(DEFAULTS, n_frames=40)
    cases = []
    p, g = zip(*[random_file(rng) for _ in range(3)])
    cases.append(('empty prediction', [[], p[1], []], list(g), small))
    cases.append(('empty ground truth', list(p), [[], g[1], []], small))
    cases.append(('both empty', [[], [], []], [[], [], []], small))
    # class 3: reference in frames 0-4, two predictions at once in frame 7 -> n_p = 2 is booked as FN; class 5 the other way round
    quirk_p = [(7, 3, 10, 0), (7, 3, 100, 0), (12, 5, 0, 0), (31, 1, 5, 5)]
    quirk_g = [(t, 3, 10, 0) for t in range(5)] + [(15, 5, 0, 0), (15, 5, 90, 0), (15, 5, -90, 30), (30, 1, 5, 5)]
    cases.append(('no common frame', [quirk_p, p[0], quirk_g], [quirk_g, g[0], quirk_p], small))
    for name, mg, mp in (('n_p > n_g', 1, 3), ('n_p < n_g', 3, 1), ('up to 2 x 2', 2, 2), ('up to 4 x 4', 4, 4)):
        fp, fg = zip(*[random_file(rng, max_g=mg, max_p=mp, density=0.3) for _ in range(3)])
        cases.append((name, list(fp), list(fg), small))
    for n_g, n_p in ((3, 1), (1, 3), (3, 3), (4, 4), (2, 4), (4, 3)):
        fp, fg = zip(*[fixed_cells(rng, n_g, n_p) for _ in range(3)])
        cases.append(('%d x %d cells' % (n_g, n_p), list(fp), list(fg), dict(DEFAULTS, n_frames=30)))
    fp, fg = zip(*[random_file(rng, max_g=3, max_p=3, density=0.3) for _ in range(4)])
    shuffle = lambda rows: [rows[i] for i in rng.permutation(len(rows))]                      # noqa: E731
    cases.append(('shuffled rows', [shuffle(r) for r in fp], [shuffle(r) for r in fg], small))
    fp, fg = zip(*[random_file(rng, max_g=2, max_p=2, density=0.3, frames=range(-5, 70)) for _ in range(3)])
    cases.append(('frames outside the range', list(fp), list(fg), small))
    for nf in (45, 50):                                      # 45: five segments, frames 45 - 49 count, 50 and later do not
        fp, fg = zip(*[random_file(rng, max_g=2, max_p=2, density=0.3, frames=range(0, 60)) for _ in range(3)])
        cases.append(('n_frames %d' % nf, list(fp), list(fg), dict(DEFAULTS, n_frames=nf)))
    for nc in (1, 14):                                       # rows of classes >= n_classes are never read
        fp, fg = zip(*[random_file(rng, n_classes=nc + 2, max_g=2, max_p=2, density=0.4) for _ in range(3)])
        cases.append(('n_classes %d' % nc, list(fp), list(fg), dict(small, n_classes=nc)))
    fp, fg = zip(*[random_file(rng, n_frames=21, n_classes=6, max_g=2, max_p=2, density=0.3) for _ in range(3)])
    cases.append(('label_rate 7', list(fp), list(fg), dict(DEFAULTS, n_frames=21, label_rate=7, n_classes=6)))
    return cases


def knife_edges():
    """-> list of (name, pred files, gt files, kwargs), one event per file in segment 0 (two frames) and a plain event in segment 1"""
    plain_g, plain_p = [(12, 4, 30, 10), (13, 4, 30, 10)], [(12, 4, 33, 12), (13, 4, 80, 12)]
    cases = []
    for thr in (20, 19.999999999999993):
        pred, gt = [], []
        for (a, b) in (KNIFE_BELOW, KNIFE_ABOVE):
            gt.append([(t, 2) + a for t in (3, 4)] + plain_g)
            pred.append([(t, 2) + b for t in (3, 4)] + plain_p)
        gt.append([(3, 2, 0, 0), (3, 2, 0, 0), (4, 2, 0, 0)] + plain_g)                        # exact duplicate reference DOAs
        pred.append([(3, 2, 5, 0), (3, 2, 50, 0), (4, 2, 5, 0)] + plain_p)
        gt.append([(3, 2, 10, 0), (3, 2, -10, 0)] + plain_g)                                  # equidistant: +-10 azimuth against 0
        pred.append([(3, 2, 0, 0)] + plain_p)
        gt.append([(3, 2, 0, 0)] + plain_g)                                                   # ... and the other way round
        pred.append([(3, 2, 10, 0), (3, 2, -10, 0)] + plain_p)
        gt.append([(3, 2, 40, 10), (3, 2, -40, 10)] + plain_g)                                # a 2 x 2 whose two pairings cost the same
        pred.append([(3, 2, 0, 10), (3, 2, 180, 10)] + plain_p)
        cases.append(('knife edges at threshold %r' % thr, pred, gt, dict(DEFAULTS, n_frames=20, doa_threshold=thr)))
    return cases


def segment_rows_of(rows, s, label_rate):
    return [r for r in rows if s * label_rate <= r[0] < (s + 1) * label_rate]


def host_segment(pred, gt, s, kw, metrics_cls=None):
    """SeldMetrics on segment s of one file alone -> (ten counters, total_DE)"""
    from salsa_amd.crnn.metrics import SeldMetrics
    m = (metrics_cls or SeldMetrics)(kw['n_classes'], kw['doa_threshold'])
    m.update(segment_rows_of(pred, s, kw['label_rate']), segment_rows_of(gt, s, kw['label_rate']), max_frames=kw['n_frames'],
             label_rate=kw['label_rate'])
    return [getattr(m, n) for n in COUNTERS], m.total_DE


def host_total(pred_files, gt_files, kw):
    """SeldMetrics over all files, the way it is used"""
    from salsa_amd.crnn.metrics import SeldMetrics
    m = SeldMetrics(kw['n_classes'], kw['doa_threshold'])
    for p, g in zip(pred_files, gt_files):
        m.update(p, g, max_frames=kw['n_frames'], label_rate=kw['label_rate'])
    return m


def segment_clearance(pred, gt, s, kw):
    """numpy's own view of how close segment s comes to a decision boundary -> (smallest gap between the best and another pairing's
    total cost over its frames, smallest |slot average - threshold|), inf where there is none; None when a cell holds more than 4."""
    from salsa_amd.crnn.metrics import angular_distance_deg, segment_rows
    from scipy.optimize import linear_sum_assignment
    lr = kw['label_rate']
    ps, gs = (segment_rows(segment_rows_of(r, s, lr), kw['n_frames'], lr)[s] for r in (pred, gt))
    gap, edge = np.inf, np.inf
    for c in range(kw['n_classes']):
        g, p = gs.get(c), ps.get(c)
        if any(len(v) > 4 for side in (g, p) if side for v in side.values()):
            return None
        if not (g and p):
            continue
        per_slot = {}
        for frame, gd in g.items():
            if frame not in p:
                continue
            ga, pa = np.array(gd, dtype=np.float64), np.array(p[frame], dtype=np.float64)
            cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
            n_g, n_p = cost.shape
            if n_g <= n_p:
                totals = sorted(sum(cost[i, m[i]] for i in range(n_g)) for m in itertools.permutations(range(n_p), n_g))
            else:
                totals = sorted(sum(cost[m[i], i] for i in range(n_p)) for m in itertools.permutations(range(n_g), n_p))
            if len(totals) > 1:
                gap = min(gap, totals[1] - totals[0])
            for r, col in zip(*linear_sum_assignment(cost)):
                per_slot.setdefault(int(r), []).append(cost[r, col])
        for d in per_slot.values():
            edge = min(edge, abs(sum(d) / len(d) - kw['doa_threshold']))
    return gap, edge


def expected_status(pred, gt, s, kw, margin):
    """2 for a cell of more than 4; 1 where numpy's costs put a rival pairing or a slot average within margin / 2; 0 where both are
    farther than 2 margin; the inputs are built so that nothing lies between (asserted here)"""
    cl = segment_clearance(pred, gt, s, kw)
    if cl is None:
        return 2
    near = min(cl)
    assert near < margin / 2 or near > 2 * margin, 'segment %d lies between margin / 2 and 2 margin (%r): rebuild the input' % (s, cl)
    return 1 if near < margin / 2 else 0
