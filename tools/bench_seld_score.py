#!/usr/bin/env python
"""Times crnn.score.score_dcase_rows (one salsa_nn_seld_score call + the host's doubt segments) and the host scorer
crnn.metrics.SeldMetrics on the SAME row set: --files (default 1024) files of 600 label frames drawn like golden g12's (14 events and
3 false alarms per file).  The device figure is wall time from rows in device memory to a finished DeviceSeldScore, median of --reps
after one warm-up; the host figure is one pass of SeldMetrics.update over the same rows already on the host (the copy of the rows it
would need first is reported separately).  Appends one JSON line to --out (default profiles/seld_score_bench.jsonl).  No ratio is
asserted: the figures are recorded as found."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def g12_like_file(rng):
    gt, pred = [], []
    for _ in range(14):
        c, t0, dur = rng.randint(12), rng.randint(0, 560), rng.randint(5, 90)
        azi, ele, fate = rng.randint(-180, 180), rng.randint(-45, 46), rng.rand()
        for t in range(t0, min(600, t0 + dur)):
            gt.append((t, c, int(azi), int(ele)))
            if fate < 0.6 or (fate > 0.8 and t > t0 + dur // 2):
                err = 8 if fate < 0.6 else 60
                a = (int(azi + rng.randint(-err, err + 1)) + 180) % 360 - 180
                pred.append((t, c, a, int(np.clip(ele + rng.randint(-err, err + 1), -90, 90))))
    for _ in range(3):
        c, t0, dur = rng.randint(12), rng.randint(0, 560), rng.randint(5, 40)
        for t in range(t0, min(600, t0 + dur)):
            pred.append((t, c, int(rng.randint(-180, 180)), int(rng.randint(-45, 46))))
    return sorted(pred, key=lambda r: r[0]), sorted(gt, key=lambda r: r[0])


def main():
    import torch
    from salsa_amd.crnn.metrics import SeldMetrics
    from salsa_amd.crnn.score import COUNTERS, DEFAULT_MARGIN, gt_rows_to_device, score_dcase_rows
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-files', type=int, default=0, help='time the host scorer on the first N files only (0: all) and scale')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seld_score_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(12)
    pred, gt = zip(*[g12_like_file(rng) for _ in range(args.files)])
    (pr, pc), (gr, gc) = gt_rows_to_device(pred, dev), gt_rows_to_device(gt, dev)
    score_dcase_rows(pr, pc, gr, gc)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = score_dcase_rows(pr, pc, gr, gc)
        times.append(time.perf_counter() - t0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    from salsa_amd.crnn.score import score_dcase_rows_async
    ev0.record()
    pending = score_dcase_rows_async(pr, pc, gr, gc)
    ev1.record()
    pending.result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows_host = pr.cpu().numpy(), pc.cpu().numpy()
    t_copy = time.perf_counter() - t0
    n_host = args.host_files or args.files
    m = SeldMetrics()
    t0 = time.perf_counter()
    for p, g in zip(pred[:n_host], gt[:n_host]):
        m.update(p, g)
    t_host = time.perf_counter() - t0
    rec = {'bench': 'seld_score', 'device': torch.cuda.get_device_name(0), 'files': args.files, 'segments': got.n_segments,
           'pred_rows': int(rows_host[1].sum()), 'margin_deg': DEFAULT_MARGIN, 'n_doubt': got.n_doubt, 'n_refused': got.n_refused,
           'device_score_s_median': float(np.median(times)), 'device_score_s_all': [round(t, 6) for t in times],
           'device_launches_ms_events': ev0.elapsed_time(ev1), 'files_per_s_device': args.files / float(np.median(times)),
           'host_files_timed': n_host, 'host_score_s': t_host, 'files_per_s_host': n_host / t_host, 'pred_rows_copy_s': t_copy}
    if n_host == args.files:
        rec['counters_equal'] = all(getattr(got, n) == getattr(m, n) for n in COUNTERS)
        rec['total_DE_diff'] = abs(got.total_DE - m.total_DE)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
