"""CPU tests of crnn/metrics.py::SeldMetrics2022, the project's restatement of the class-wise DCASE 2022 SELD metric (DESIGN.md
section 9t): against the pinned 2021 scorer SeldMetrics on golden g12 and every built family (the class sums ARE its counters), on
hand-computed cases, and its classwise(), merge(), file_records() and jackknife(); evaluate_csv_dirs and the row writers for '2022'."""
import csv
import os

import numpy as np
import pytest

import seld_score_cases as cases
import seld_score2022_cases as cases22

EPS = np.finfo(float).eps
INPUTS = [('g12',) + cases.g12_files() + (cases.DEFAULTS,)] + cases.built_families()


@pytest.mark.parametrize('k', range(len(INPUTS)), ids=[c[0].replace(' ', '_') for c in INPUTS])
def test_class_sums_are_the_pinned_scorers_counters(k):
    name, pred, gt, kw = INPUTS[k]
    old = cases.host_total(pred, gt, kw)
    m = cases22.host_total(pred, gt, kw, 'micro')
    assert (int(m.TP.sum()), int(m.FP.sum() + m.FP_spatial.sum()), int(m.FN.sum()), int(m.Nref.sum())) == (old.TP, old.FP, old.FN, old.Nref)
    assert (int(m.DE_TP.sum()), int(m.DE_FP.sum()), int(m.DE_FN.sum()), m.S, m.D, m.I) == (old.DE_TP, old.DE_FP, old.DE_FN, old.S, old.D, old.I)
    # non-negative terms added in another order: the relative error of either sum is at most (terms - 1) x 2^-53, so the two differ
    # by at most DE_TP x 2^-52 relative
    assert abs(m.total_DE.sum() - old.total_DE) <= old.DE_TP * 2.0 ** -52 * old.total_DE
    assert (m.FP == m.DE_FP).all() and (m.FN == m.DE_FN).all() and (m.FP_spatial == m.DE_TP - m.TP).all()
    assert all(getattr(m, n).shape == (kw['n_classes'],) and getattr(m, n).dtype == np.int64 for n in cases22.EIGHT) and m.total_DE.dtype == np.float64
    ER, F, LE, LR = m.scores()
    oER, oF, oLE, oLR = old.scores()
    assert (ER, LE, LR) == pytest.approx((oER, oLE, oLR), rel=1e-12, abs=1e-12)
    # the one difference: the slot averages above the threshold weigh 1 in F, not 1/2
    sp = int(m.FP_spatial.sum())
    assert F == pytest.approx(old.TP / (EPS + old.TP + sp + 0.5 * (old.FP - sp + old.FN)), rel=1e-12, abs=1e-12)
    if sp and old.TP:
        assert F < oF
    macro = cases22.host_total(pred, gt, kw)
    assert macro.classwise().shape == (kw['n_classes'], 5)
    assert macro.classwise().mean(axis=0) == pytest.approx((ER,) + macro.scores()[1:] + (macro.seld_error(),), rel=1e-12)


def scorer(pred, gt, n_classes=3, average='macro', **kw):
    from salsa_amd.crnn.metrics import SeldMetrics2022
    m = SeldMetrics2022(n_classes, 20, average)
    m.update(pred, gt, max_frames=10, **kw)
    return m


def test_hand_computed_scores():
    # class 0: a hit 10 degrees off; class 1: ground truth only (DE_TP == 0 -> LE 180); class 2: absent from both sides
    m = scorer([(0, 0, 10, 0)], [(0, 0, 0, 0), (1, 1, 0, 0)])
    assert [list(getattr(m, n)) for n in ('TP', 'FN', 'Nref', 'DE_TP', 'DE_FN')] == [[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 1, 0]]
    assert (m.S, m.D, m.I) == (0, 1, 0) and m.total_DE[0] == pytest.approx(10.0, abs=1e-9)
    cw = m.classwise()
    assert cw[:, 0] == pytest.approx([0.5] * 3) and cw[:, 1] == pytest.approx([1, 0, 0]) and cw[:, 3] == pytest.approx([1, 0, 0])
    assert cw[:, 2] == pytest.approx([10, 180, 180]) and list(cw[1:, 2]) == [180, 180]
    assert cw[:, 4] == pytest.approx([(0.5 + 0 + 10 / 180 + 0) / 4, (0.5 + 1 + 1 + 1) / 4, (0.5 + 1 + 1 + 1) / 4])
    assert m.scores() == pytest.approx((0.5, 1 / 3, 370 / 3, 1 / 3)) and m.seld_error() == pytest.approx(cw[:, 4].mean())
    micro = scorer([(0, 0, 10, 0)], [(0, 0, 0, 0), (1, 1, 0, 0)], average='micro')
    assert micro.scores() == pytest.approx((0.5, 1 / 1.5, 10.0, 0.5)) and micro.seld_error() == pytest.approx((0.5 + 1 / 3 + 10 / 180 + 0.5) / 4)


def test_a_slot_average_just_above_the_threshold_lands_in_fp_spatial():
    below, above = scorer([(0, 0) + cases.KNIFE_BELOW[1]], [(0, 0) + cases.KNIFE_BELOW[0]]), scorer([(0, 0) + cases.KNIFE_ABOVE[1]], [(0, 0) + cases.KNIFE_ABOVE[0]])
    assert (below.TP[0], below.FP_spatial[0], below.FP[0], below.I) == (1, 0, 0, 0)
    assert (above.TP[0], above.FP_spatial[0], above.FP[0], above.DE_TP[0], above.DE_FP[0]) == (0, 1, 0, 1, 0) and (above.S, above.D, above.I) == (0, 0, 1)
    # F_0 = 0 / (0 + 1 + 0), LR_0 = 1 / (1 + 0), LE_0 = 20.00000000000001; ER = 1 / 1
    assert above.classwise()[0] == pytest.approx([1, 0, 20.00000000000001, 1, (1 + 1 + 20.00000000000001 / 180 + 0) / 4])


def test_count_excess_on_either_side_and_no_common_frame():
    more = scorer([(0, 0, 0, 0), (0, 0, 90, 0), (0, 0, -90, 0)], [(0, 0, 1, 0)])                  # n_p = 3 > n_g = 1
    assert (more.TP[0], more.FP[0], more.DE_FP[0], more.FP_spatial[0], more.FN[0], more.Nref[0]) == (1, 2, 2, 0, 0, 1) and (more.S, more.D, more.I) == (0, 0, 2)
    assert more.classwise()[0, 1] == pytest.approx(1 / (1 + 0.5 * 2)) and more.scores()[0] == pytest.approx(2.0)
    fewer = scorer([(0, 0, 0, 0)], [(0, 0, 1, 0), (0, 0, 90, 0), (0, 0, -90, 0)])                 # n_p = 1 < n_g = 3
    assert (fewer.TP[0], fewer.FN[0], fewer.DE_FN[0], fewer.FP[0], fewer.Nref[0], fewer.DE_TP[0]) == (1, 2, 2, 0, 3, 1) and (fewer.S, fewer.D, fewer.I) == (0, 2, 0)
    assert fewer.classwise()[0, 1] == pytest.approx(1 / 2) and fewer.classwise()[0, 3] == pytest.approx(1 / 3)
    # both sides hold class 1 but in no common frame: the PREDICTED count (2) is booked as misses, Nref counts the reference's 1
    apart = scorer([(5, 1, 0, 0), (5, 1, 90, 0)], [(2, 1, 0, 0)])
    assert (apart.FN[1], apart.DE_FN[1], apart.Nref[1], apart.DE_TP[1], apart.FP[1], apart.TP[1]) == (2, 2, 1, 0, 0, 0) and (apart.S, apart.D, apart.I) == (0, 2, 0)
    assert apart.classwise()[1] == pytest.approx([2, 0, 180, 0, (2 + 1 + 1 + 1) / 4])


def three_files():
    name, pred, gt, kw = cases22.main_case()
    return pred[:2] + [pred[0][::2] + pred[1][1::2]], gt[:2] + [gt[1]], kw


@pytest.mark.parametrize('average', ['macro', 'micro'])
def test_merge_file_records_and_jackknife(average):
    from salsa_amd.crnn.metrics import SeldMetrics2022
    from scipy import stats
    pred, gt, kw = three_files()
    new = lambda: SeldMetrics2022(kw['n_classes'], kw['doa_threshold'], average)               # noqa: E731
    feed = lambda m, fs: [m.update(pred[f], gt[f], max_frames=kw['n_frames'], label_rate=kw['label_rate']) for f in fs] and m   # noqa: E731
    whole = feed(new(), [0, 1, 2])
    merged = feed(new(), [0]).merge(feed(new(), [1, 2]))
    rec, rec_m = whole.file_records(), merged.file_records()
    assert rec['TP'].shape == (3, kw['n_classes']) and rec['S'].shape == (3,) and rec['total_DE'].shape == (3, kw['n_classes'])
    for n in cases22.EIGHT + ('S', 'D', 'I', 'total_DE'):
        assert (rec[n] == rec_m[n]).all(), n
        assert (rec[n].sum(axis=0) == getattr(whole, n)).all() or n == 'total_DE', n
        assert np.array_equal(np.asarray(getattr(merged, n)), np.asarray(getattr(whole, n))) or n == 'total_DE', n
    assert merged.total_DE == pytest.approx(whole.total_DE, rel=1e-14) and merged.scores() == pytest.approx(whole.scores(), rel=1e-12)
    with pytest.raises(ValueError, match='merge'):
        whole.merge(SeldMetrics2022(kw['n_classes'] + 1))
    # a direct leave-one-out recomputation with fresh scorers
    full = np.array(whole.scores() + (whole.seld_error(),))
    loo = np.array([(lambda m: m.scores() + (m.seld_error(),))(feed(new(), [f for f in range(3) if f != i])) for i in range(3)])
    assert np.ptp(loo[:, 4]) > 1e-3                                                            # the files differ: the interval is not a point
    bias = 2 * (loo.mean(axis=0) - full)
    se = np.sqrt(2 / 3 * ((loo - loo.mean(axis=0)) ** 2).sum(axis=0))
    q = stats.t.ppf(0.975, 2)
    jk = whole.jackknife()
    assert list(jk) == ['ER', 'F', 'LE', 'LR', 'SELD']
    for k, name in enumerate(jk):
        est, b, s, (lo, hi) = jk[name]
        # (the totals minus a file against a fresh sum of the other two: float64 subtraction, a few ulps of total_DE)
        assert (est, b, s, lo, hi) == pytest.approx((full[k] - bias[k], bias[k], se[k], full[k] - bias[k] - q * se[k], full[k] - bias[k] + q * se[k]),
                                                    rel=1e-9, abs=1e-10), name
    wide, narrow = whole.jackknife(0.99)['SELD'][3], whole.jackknife(0.5)['SELD'][3]
    assert wide[0] < jk['SELD'][3][0] < narrow[0] < narrow[1] < jk['SELD'][3][1] < wide[1]
    with pytest.raises(ValueError, match='at least 2 files'):
        feed(new(), [0]).jackknife()
    with pytest.raises(ValueError, match='average'):
        SeldMetrics2022(4, 20, 'weighted')


def test_macro_and_micro_differ_on_unbalanced_classes():
    pred, gt, kw = three_files()
    a, b = cases22.host_total(pred, gt, kw, 'macro'), cases22.host_total(pred, gt, kw, 'micro')
    assert a.scores()[0] == b.scores()[0] and abs(a.seld_error() - b.seld_error()) > 1e-3 and (a.classwise() == b.classwise()).all()


def test_evaluate_csv_dirs_and_the_row_layout_of_2022(tmp_path):
    from salsa_amd.crnn.decode import rows_to_list
    from salsa_amd.crnn.metrics import SeldMetrics2022, evaluate_csv_dirs, load_dcase_csv
    from salsa_amd.crnn.postprocess import multi_accdoa_rows, to_dcase_rows
    import salsa_amd.crnn.metrics as metrics
    assert metrics.SeldMetrics2022 is SeldMetrics2022 and all(hasattr(metrics, n) for n in ('SeldMetrics', 'SeldMetrics2020'))
    pred, gt, kw = three_files()
    names = ['mix%d.csv' % f for f in range(3)]
    for d, files in (('pred', pred), ('gt', gt)):
        os.makedirs(str(tmp_path / d))
        for fn, rows in zip(names, files):
            with open(str(tmp_path / d / fn), 'w', newline='') as f:
                csv.writer(f).writerows([(r[0], r[1], 0, r[2], r[3]) for r in rows])           # the 2021 layout: a track column
    assert load_dcase_csv(str(tmp_path / 'gt' / names[0]), version='2022') == load_dcase_csv(str(tmp_path / 'gt' / names[0]), version='2021')
    args = (str(tmp_path / 'pred'), str(tmp_path / 'gt'), names, kw['n_classes'], kw['doa_threshold'], kw['n_frames'], kw['label_rate'])
    for average in ('macro', 'micro'):
        m = cases22.host_total(pred, gt, kw, average)
        assert evaluate_csv_dirs(*args, eval_version='2022', average=average) == m.scores() + (m.seld_error(),)
    assert evaluate_csv_dirs(*args, eval_version='2022') == evaluate_csv_dirs(*args, eval_version='2022', average='macro')
    old = cases.host_total(pred, gt, kw)
    assert evaluate_csv_dirs(*args) == old.scores() + (old.seld_error(),)                      # '2021' as before
    for bad in ('2019', '2023', 2022):
        with pytest.raises(ValueError, match='Unknown eval_version'):
            evaluate_csv_dirs(*args, eval_version=bad)
    with pytest.raises(ValueError, match='not implemented'):
        load_dcase_csv(str(tmp_path / 'gt' / names[0]), version='2019')
    # the row writers: '2022' is the 2021 layout [frame, class, 0, azimuth, elevation]
    rng = np.random.RandomState(3)
    prob, xyz = rng.rand(20, 12), rng.randn(20, 36)
    assert to_dcase_rows(prob, xyz, max_nframes_per_file=20, eval_version='2022') == to_dcase_rows(prob, xyz, max_nframes_per_file=20, eval_version='2021')
    assert len(to_dcase_rows(prob, xyz, max_nframes_per_file=20, eval_version='2022')[0]) == 5
    act, vec = rng.rand(20, 36).astype(np.float32), rng.randn(20, 108).astype(np.float32)
    multi = multi_accdoa_rows(act, vec, max_nframes_per_file=20, eval_version='2022')
    assert multi == multi_accdoa_rows(act, vec, max_nframes_per_file=20, eval_version='2021') and len(multi[0]) == 5 and multi[0][2] == 0
    rows, counts = np.array([[[3, 1, 40, -5], [4, 2, 7, 8]]], dtype=np.int16), np.array([2], dtype=np.int32)
    assert rows_to_list(rows, counts, eval_version='2022') == rows_to_list(rows, counts, eval_version='2021') == [[[3, 1, 0, 40, -5], [4, 2, 0, 7, 8]]]
