"""crnn/metrics.py::SeldMetrics2020, the host scorer of the SELD 2020 metric, against golden g29: the reference's own
metrics/SELD2020_evaluation_metrics.py on golden g12's file pairs and every built family and knife edge of tests/seld_score_cases.py
(tools/make_golden_metrics2020.py), cumulatively file by file.

Bounds.  The ten integers are EQUAL.  |total_DE - fixture| <= 4e-12 x DE_TP degrees: a class average is a mean of sums of at most four
distances, and numpy's arccos differs from one machine's dispatch to another's by at most 7.2e-13 degrees per distance (measured;
tests/test_seld_score_cpu.py), four times that rounded up as NUMPY_ACOS_DEG is there.  Scores and the seld error to 1e-12."""
import os

import numpy as np
import pytest

import seld_score_cases as cases
import seld_score2020_cases as cases20
from conftest import load_golden


@pytest.fixture(scope='module')
def g29():
    """-> list of (name, pred files, gt files, kwargs, cumulative counters (n_files, 11), scores (n_files, 5)) from the fixture's own rows"""
    meta, a = load_golden('g29_metrics2020')
    assert meta['columns'].split() == list(cases20.COUNTERS) + ['total_DE']
    out = []
    for k, c in enumerate(meta['cases']):
        files = {side: [[tuple(int(v) for v in r[1:]) for r in a['c%d_%s' % (k, side)] if r[0] == f] for f in range(c['n_files'])]
                 for side in ('pred', 'gt')}
        out.append((c['name'], files['pred'], files['gt'], c['kwargs'], a['c%d_cumulative' % k], a['c%d_scores' % k]))
    return out


def test_fixture_holds_g12_every_built_family_and_the_knife_edges(g29):
    want = [('g12',) + cases.g12_files() + (cases.DEFAULTS,)] + cases.built_families() + cases.knife_edges()
    assert [c[0] for c in g29] == [c[0] for c in want]
    for (name, pred, gt, kw, _, _), (_, wp, wg, wkw) in zip(g29, want):
        assert pred == [list(map(tuple, f)) for f in wp] and gt == [list(map(tuple, f)) for f in wg] and kw == wkw, name
    assert {'shuffled rows', 'n_classes 14'} <= {c[0] for c in g29}
    # the reference's own numbers for g12 (12 classes, 20 degrees): TP FP FN . . . . Nref Nsys DE_TP total_DE
    last = g29[0][4][-1]
    assert [last[i] for i in (0, 1, 2, 7, 8, 9)] == [113, 37, 177, 290, 219, 182] and last[10] == pytest.approx(3769.600769, abs=1e-6)
    assert g29[0][5][-1][:4] == pytest.approx([0.6586, 0.4440, 20.7121, 0.7151], abs=5e-5)


def test_counters_total_de_and_scores_cumulatively(g29):
    from salsa_amd.crnn.metrics import SeldMetrics2020
    for name, pred, gt, kw, cum, scores in g29:
        m = SeldMetrics2020(kw['n_classes'], kw['doa_threshold'])
        for f, (p, g) in enumerate(zip(pred, gt)):
            m.update(p, g, max_frames=kw['n_frames'], label_rate=kw['label_rate'])
            what = '%s: after file %d' % (name, f)
            assert [getattr(m, n) for n in cases20.COUNTERS] == list(cum[f, :10]), what
            assert abs(m.total_DE - cum[f, 10]) <= cases20.NUMPY_ACOS_DEG4 * m.DE_TP, what
            if m.Nref > 0:
                assert np.abs(np.array(m.scores() + (m.seld_error(),)) - scores[f]).max() <= 1e-12, what
            else:
                assert np.isnan(scores[f]).all(), what


def test_shuffled_rows_score_as_the_sorted_ones(g29):
    """ascending frame order: the reference segments by walking the audio frames, so the order of the rows between frames is nothing"""
    from salsa_amd.crnn.metrics import SeldMetrics2020
    name, pred, gt, kw, cum, _ = next(c for c in g29 if c[0] == 'shuffled rows')
    by_frame = lambda rows: sorted(rows, key=lambda r: r[0])                     # noqa: E731  (stable: DOAs of a frame keep file order)
    a, b = SeldMetrics2020(kw['n_classes'], kw['doa_threshold']), SeldMetrics2020(kw['n_classes'], kw['doa_threshold'])
    for p, g in zip(pred, gt):
        assert p != by_frame(p)
        a.update(p, g, max_frames=kw['n_frames'])
        b.update(by_frame(p), by_frame(g), max_frames=kw['n_frames'])
    assert vars(a) == vars(b) and a.DE_TP > 100


def test_a_segment_scored_alone_is_its_share_of_the_file(g29):
    """what the host's resolution of doubt segments relies on (alone: as a file of that one segment, for every class of an empty
    segment is a true negative): the integers add up exactly; total_DE is the same class averages
    added segment by segment first, so the two sums differ by rounding alone: each makes at most DE_TP additions, each within half
    a spacing of the total"""
    from salsa_amd.crnn.metrics import SeldMetrics2020
    for name, pred, gt, kw, _, _ in g29:
        n_seg = -(-kw['n_frames'] // kw['label_rate'])
        for p, g in zip(pred, gt):
            whole = SeldMetrics2020(kw['n_classes'], kw['doa_threshold'])
            whole.update(p, g, max_frames=kw['n_frames'], label_rate=kw['label_rate'])
            parts = [cases20.host_segment(p, g, s, kw) for s in range(n_seg)]
            assert [sum(c[i] for c, _ in parts) for i in range(10)] == [getattr(whole, n) for n in cases20.COUNTERS], name
            assert abs(sum(de for _, de in parts) - whole.total_DE) <= whole.DE_TP * np.spacing(whole.total_DE), name


def test_evaluate_csv_dirs_by_version(g29, tmp_path):
    from salsa_amd.crnn.metrics import SeldMetrics, evaluate_csv_dirs
    from salsa_amd.crnn.postprocess import write_dcase_csv
    name, pred, gt, kw, _, scores = g29[0]
    (tmp_path / 'pred').mkdir()
    (tmp_path / 'gt').mkdir()
    names = ['f%d.csv' % f for f in range(len(pred))]
    for fn, p, g in zip(names, pred, gt):
        write_dcase_csv(str(tmp_path / 'pred' / fn), p)                                             # 4 columns: the 2020 submission rows
        write_dcase_csv(str(tmp_path / 'gt' / fn), [(t, c, 0, azi, ele) for t, c, azi, ele in g])   # 5 columns: with a track
    dirs = (str(tmp_path / 'pred'), str(tmp_path / 'gt'), names)
    got = evaluate_csv_dirs(*dirs, eval_version='2020')
    assert np.abs(np.array(got) - scores[-1]).max() <= 1e-12
    m = SeldMetrics()
    for p, g in zip(pred, gt):
        m.update(p, g)
    assert evaluate_csv_dirs(*dirs) == evaluate_csv_dirs(*dirs, eval_version='2021') == m.scores() + (m.seld_error(),)
    assert got != evaluate_csv_dirs(*dirs)
    for bad in ('2019', 2020, None):
        with pytest.raises(ValueError, match='Unknown eval_version'):
            evaluate_csv_dirs(*dirs, eval_version=bad)
    assert os.listdir(str(tmp_path / 'pred')) != []


def test_an_empty_reference_does_not_raise():
    from salsa_amd.crnn.metrics import SeldMetrics2020
    m = SeldMetrics2020()
    assert m.scores() == (0.0, 0.0, 180, 0.0) and m.seld_error() == (0.0 + 1.0 + 1.0 + 1.0) / 4
    m.update([(3, 1, 10, 0), (3, 1, 50, 0), (14, 2, 0, 0)], [], max_frames=20)
    assert (m.Nref, m.Nsys, m.FP, m.TN, m.I, m.DE_TP) == (0, 2, 2, 22, 2, 0)
    ER, F, LE, LR = m.scores()
    assert ER == 2 / np.finfo(float).eps and F == 0.0 and LE == 180 and LR == 0.0 and np.isfinite(m.seld_error())
