#!/usr/bin/env python
"""Generate tests/golden/g29_metrics2020.npz: the UPSTREAM reference's SELD 2020 scorer (metrics/SELD2020_evaluation_metrics.py
SELDMetrics.update_seld_scores / compute_seld_scores with metrics/dcase_utils.py, imported unmodified from the reference checkout
given as --reference) on the row sets the scoring tests use: golden g12's four file pairs and every case of
tests/seld_score_cases.py::built_families() and knife_edges().  Run:  python tools/make_golden_metrics2020.py --reference DIR

The path is the one models/interfaces.py:163-180 takes: every row list is written to a CSV (predictions in the 4-column submission
form, ground truth in the 5-column form with a zero track), read back with load_output_format_file(version='2020'), segmented with
segment_labels and handed to update_seld_scores.  Per case the fixture holds the input rows, (file, frame, class, azimuth,
elevation) int16, and the eleven counters TP FP FN TN S D I Nref Nsys DE_TP total_DE cumulatively after every file; where Nref > 0
also ER F LE LR and the seld error (interfaces.py:179), NaN elsewhere: compute_seld_scores raises ZeroDivisionError on an empty
reference (its unused aux_metrics list divides Nsys / Nref).  The module imports under numpy 2 only with numpy.float restored and a
stand-in for IPython (imported, never called), as tools/make_golden.py::g12_metrics arranges for the 2021 twin.  Data only."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COLUMNS = 'TP FP FN TN S D I Nref Nsys DE_TP total_DE'


def write_csv(path, rows, with_track):
    with open(path, 'w') as f:
        for t, c, azi, ele in rows:
            f.write(('%d,%d,0,%d,%d\n' if with_track else '%d,%d,%d,%d\n') % (t, c, azi, ele))


def score_case(M, U, pred_files, gt_files, kw, tmp):
    """-> (cumulative counters (n_files, 11), cumulative scores (n_files, 5), NaN where the reference has none)"""
    ev = M.SELDMetrics(nb_classes=kw['n_classes'], doa_threshold=kw['doa_threshold'])
    cum, scores = [], []
    for pred, gt in zip(pred_files, gt_files):
        write_csv(os.path.join(tmp, 'pred.csv'), pred, False)
        write_csv(os.path.join(tmp, 'gt.csv'), gt, True)
        p, g = (U.segment_labels(U.load_output_format_file(os.path.join(tmp, n), version='2020'), _max_frames=kw['n_frames'],
                                 _nb_label_frames_1s=kw['label_rate']) for n in ('pred.csv', 'gt.csv'))
        ev.update_seld_scores(p, g)
        cum.append([float(v) for v in (ev._TP, ev._FP, ev._FN, ev._TN, ev._S, ev._D, ev._I, ev._Nref, ev._Nsys, ev._DE_TP, ev._total_DE)])
        if ev._Nref > 0:
            ER, F, LE, LR = (float(v) for v in ev.compute_seld_scores())
            scores.append([ER, F, LE, LR, (ER + (1.0 - F) + LE / 180.0 + (1.0 - LR)) / 4])       # interfaces.py:179
        else:
            scores.append([np.nan] * 5)
    return np.array(cum), np.array(scores)


def with_file_column(files):
    rows = [(f,) + tuple(r) for f, file_rows in enumerate(files) for r in file_rows]
    return np.array(rows, dtype=np.int16).reshape(-1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the upstream repository')
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), args.reference]
    sys.modules.setdefault('IPython', types.SimpleNamespace(embed=lambda *a, **k: None))   # imported, never called
    if not hasattr(np, 'float'):
        np.float = float                                                                    # (removed in numpy 1.24; the module's eps)
    from metrics import SELD2020_evaluation_metrics as M, dcase_utils as U
    import seld_score_cases as cases
    all_cases = [('g12',) + cases.g12_files() + (cases.DEFAULTS,)] + cases.built_families() + cases.knife_edges()
    tmp = tempfile.mkdtemp()
    meta, arrays = {'columns': COLUMNS, 'score_columns': 'ER F LE LR seld_error', 'row_columns': 'file frame class azimuth elevation',
                    'cases': []}, {}
    for k, (name, pred, gt, kw) in enumerate(all_cases):
        cum, scores = score_case(M, U, pred, gt, kw, tmp)
        meta['cases'].append({'name': name, 'n_files': len(pred), 'kwargs': kw})
        arrays.update({'c%d_pred' % k: with_file_column(pred), 'c%d_gt' % k: with_file_column(gt), 'c%d_cumulative' % k: cum,
                       'c%d_scores' % k: scores})
        print('%-44s %s' % (name, ' '.join('%g' % v for v in cum[-1])))
    shutil.rmtree(tmp)
    path = os.path.join(ROOT, 'tests', 'golden', 'g29_metrics2020.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print('%s: %.1f KB, %d cases' % (path, os.path.getsize(path) / 1024, len(all_cases)))


if __name__ == '__main__':
    main()
