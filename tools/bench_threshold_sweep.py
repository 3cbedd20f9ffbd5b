#!/usr/bin/env python
"""Times the one-launch threshold sweep (crnn.calibrate.sweep_outputs, salsa_nn_seld_sweep) against the composed path it replaces --
K x (decode_dcase_rows | decode_multi_rows, then score_dcase_rows(eval_version='2022')), what SALSA_HIP_SWEEP=0 runs -- on the SAME
combined file outputs: --files (default 32) files x 600 label frames x 12 classes, K = --candidates (default 17) thresholds from 0.1
to 0.9, for output_format 'reg_xyz' and 'multi_accdoa'.  The inputs are drawn like the test suite's random case: activities uniform in
[0.1, 0.95], random directions, a reference near the (first track's) predicted direction in 40 % of the cells.

After a warm-up of both and after both were held to each other (integers equal, total_DE within DE_TP x margin), the two legs
ALTERNATE in one process; a sample is the wall time of one whole call (launches, copies to pinned memory, the host's share: the
resolution of doubt entries and the unpacking), --samples (default 15) samples of each.  The median and the range (min - max) are
recorded; for the sweep the launch alone (both kernels between two device events, mean of --inner calls) is recorded next to them,
so that where the time goes can be read off.  Appends one JSON line per format to --out (default
profiles/threshold_sweep_bench.jsonl).  No ratio is asserted: the figures are recorded as found."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_outputs(seed, n_files, n_frames, n_classes, multi, gt_density=0.4):
    rng = np.random.RandomState(seed)
    tracks = 3 if multi else 1
    act = rng.uniform(0.1, 0.95, (n_files, n_frames, tracks * n_classes)).astype(np.float32)
    v = rng.standard_normal((n_files, n_frames, 3, tracks, n_classes)).astype(np.float32)
    first = np.moveaxis(v[:, :, :, 0, :], 2, -1).astype(np.float64)
    azi = np.around(np.degrees(np.arctan2(first[..., 1], first[..., 0]))).astype(np.int64)
    ele = np.around(np.degrees(np.arctan2(first[..., 2], np.hypot(first[..., 0], first[..., 1])))).astype(np.int64)
    gt = []
    for f in range(n_files):
        rows = []
        for t, c in zip(*np.nonzero(rng.uniform(size=(n_frames, n_classes)) < gt_density)):
            rows.append((int(t), int(c), (int(azi[f, t, c]) + int(rng.randint(-30, 31)) + 180) % 360 - 180,
                         int(np.clip(int(ele[f, t, c]) + int(rng.randint(-10, 11)), -90, 90))))
        gt.append(rows)
    return act, v.reshape(n_files, n_frames, 3 * tracks * n_classes), gt


def main():
    import torch
    from salsa_amd.crnn import calibrate
    from salsa_amd.crnn.score import DEFAULT_MARGIN, gt_rows_to_device
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--candidates', type=int, default=17)
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'threshold_sweep_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    n_frames, nc = 600, 12
    thresholds = np.linspace(0.1, 0.9, args.candidates, dtype=np.float32)
    spread = lambda v: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}     # noqa: E731
    for fmt in ('reg_xyz', 'multi_accdoa'):
        act, xyz, gt = random_outputs(7, args.files, n_frames, nc, fmt == 'multi_accdoa')
        act, xyz = torch.from_numpy(act).to(dev), torch.from_numpy(xyz).to(dev)
        gt_rows, gt_counts = gt_rows_to_device(gt, dev)
        kw = dict(n_frames=n_frames, n_classes=nc, output_format=fmt)

        def leg(composed):
            os.environ['SALSA_HIP_SWEEP'] = '0' if composed else '1'
            try:
                return calibrate.sweep_outputs(act, xyz, gt_rows, gt_counts, thresholds, **kw)
            finally:
                os.environ.pop('SALSA_HIP_SWEEP')
        for _ in range(3):
            one, many = leg(False), leg(True)
        equal = bool((one.counters == many.counters).all())
        de_ok = bool((np.abs(one.total_DE - many.total_DE) <= one.counters[..., 5] * DEFAULT_MARGIN).all())
        wall = {False: [], True: []}
        for _ in range(args.samples):
            for composed in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(composed)
                wall[composed].append((time.perf_counter() - t0) * 1e3)
        launch = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pending = [calibrate.PendingSweep(act, xyz, gt_rows, gt_counts, thresholds, n_frames, nc, 20, 10, DEFAULT_MARGIN, fmt, 15.0)
                       for _ in range(args.inner)]
            e1.record()
            torch.cuda.synchronize()
            launch.append(e0.elapsed_time(e1) / args.inner)               # (launch, both kernels and the copies to pinned memory)
            del pending
        chosen, index = one.best()
        rec = {'bench': 'threshold_sweep', 'device': torch.cuda.get_device_name(0), 'output_format': fmt, 'files': args.files,
               'label_frames': n_frames, 'classes': nc, 'candidates': args.candidates, 'samples': args.samples, 'margin_deg': DEFAULT_MARGIN,
               'entries': one.n_entries, 'n_doubt': one.n_doubt, 'n_refused': one.n_refused, 'composed_doubt_segments': many.n_doubt,
               'counters_equal': equal, 'total_DE_within_margin': de_ok, 'chosen_indices': [int(i) for i in index],
               'sweep_outputs_wall_ms': spread(wall[False]), 'composed_wall_ms': spread(wall[True]),
               'sweep_issue_and_device_ms': spread(launch)}
        rec['wall_median_ratio_composed_over_sweep'] = rec['composed_wall_ms']['median'] / rec['sweep_outputs_wall_ms']['median']
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        print(json.dumps(rec))


if __name__ == '__main__':
    main()
