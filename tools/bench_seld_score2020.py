#!/usr/bin/env python
"""Times salsa_nn_seld_score2020 next to salsa_nn_seld_score on the SAME rows: --files (default 32) files of 600 label frames drawn
like golden g12's (tools/bench_seld_score.py::g12_like_file).  Each figure is one call of the export (the per-segment kernel and the
sum kernel) between two device events on the current stream, the two exports ALTERNATING for --reps calls each after a warm-up of
both; the median, the quartiles and the extremes are recorded.  The wall time of crnn.score.score_dcase_rows (launch, copies, the
host's doubt segments) is recorded for both versions too, and the 2020 result is held against SeldMetrics2020 on the host.  Appends
one JSON line to --out (default profiles/seld_score2020_bench.jsonl).  No ratio is asserted: the figures are recorded as found."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    import torch
    from bench_seld_score import g12_like_file
    from salsa_amd import _lib
    from salsa_amd.crnn.metrics import SeldMetrics2020
    from salsa_amd.crnn.score import COUNTERS_2020, DEFAULT_MARGIN, gt_rows_to_device, score_dcase_rows
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seld_score2020_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(12)
    pred, gt = zip(*[g12_like_file(rng) for _ in range(args.files)])
    (pr, pc), (gr, gc) = gt_rows_to_device(pred, dev), gt_rows_to_device(gt, dev)
    n_seg = 60
    counters = torch.empty((args.files * n_seg, 10), dtype=torch.int32, device=dev)
    de = torch.empty((args.files * n_seg,), dtype=torch.float64, device=dev)
    status = torch.empty((args.files * n_seg,), dtype=torch.int32, device=dev)
    sums, sum_de = torch.empty((10,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(name):
        rc = getattr(L, name)(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], args.files, 600, 10, 12, 20.0, DEFAULT_MARGIN,
                              ptr(counters), ptr(de), ptr(status), ptr(sums), ptr(sum_de), stream)
        assert rc == 0, (name, rc)
    names = ('salsa_nn_seld_score', 'salsa_nn_seld_score2020')
    for _ in range(10):
        for n in names:
            call(n)
    torch.cuda.synchronize()
    events = {n: [] for n in names}
    for _ in range(args.reps):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(n)
            e1.record()
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    ms = {n: np.array([a.elapsed_time(b) for a, b in events[n]]) for n in names}
    wall = {}
    for version in ('2021', '2020'):
        score_dcase_rows(pr, pc, gr, gc, eval_version=version)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            got = score_dcase_rows(pr, pc, gr, gc, eval_version=version)
            t.append(time.perf_counter() - t0)
        wall[version] = float(np.median(t))
    m = SeldMetrics2020()
    for p, g in zip(pred, gt):
        m.update(p, g)
    rec = {'bench': 'seld_score2020', 'device': torch.cuda.get_device_name(0), 'files': args.files, 'segments': got.n_segments,
           'pred_rows': int(pc.sum()), 'gt_rows': int(gc.sum()), 'reps': args.reps, 'margin_deg': DEFAULT_MARGIN,
           'n_doubt_2020': got.n_doubt, 'n_refused_2020': got.n_refused,
           'counters_equal_2020': all(getattr(got, n) == getattr(m, n) for n in COUNTERS_2020), 'total_DE_diff_2020': abs(got.total_DE - m.total_DE),
           'score_dcase_rows_wall_s_2021': wall['2021'], 'score_dcase_rows_wall_s_2020': wall['2020']}
    for n in names:
        q = np.percentile(ms[n], [0, 25, 50, 75, 100])
        rec[n + '_ms'] = {'min': q[0], 'q25': q[1], 'median': q[2], 'q75': q[3], 'max': q[4]}
    rec['median_ratio_2020_over_2021'] = float(np.median(ms[names[1]]) / np.median(ms[names[0]]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
