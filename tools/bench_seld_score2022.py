#!/usr/bin/env python
"""Times salsa_nn_seld_score2022 next to the unchanged salsa_nn_seld_score on the SAME rows: --files (default 32) files of 600 label
frames drawn like golden g12's (tools/bench_seld_score.py::g12_like_file).  After a warm-up of both, the two calls ALTERNATE in one
process; a sample is the mean over --inner back-to-back calls between two device events, and --samples (default 7) samples are
taken of each: "launch alone" is the export itself (the per-segment kernel and its sum kernel), "whole call" the wall time of
crnn.score.score_dcase_rows (launch, copies to pinned memory, the host's share).  The median (min - max) of the samples is recorded
and the 2022 result is held against SeldMetrics2022 on the host.  Appends one JSON line to --out (default
profiles/seld_score2022_bench.jsonl).  No ratio is asserted: the 2021 call is the yardstick and the figures are recorded as found."""
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
    from salsa_amd.crnn.metrics import SeldMetrics2022
    from salsa_amd.crnn.score import DEFAULT_MARGIN, gt_rows_to_device, score_dcase_rows
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=32)
    ap.add_argument('--samples', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seld_score2022_bench.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(12)
    pred, gt = zip(*[g12_like_file(rng) for _ in range(args.files)])
    (pr, pc), (gr, gc) = gt_rows_to_device(pred, dev), gt_rows_to_device(gt, dev)
    n_seg, nc, n = 60, 12, args.files
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)       # noqa: E731
    outs = {'salsa_nn_seld_score': (new((n * n_seg, 10), torch.int32), new((n * n_seg,), torch.float64), new((n * n_seg,), torch.int32),
                                    new((10,), torch.int64), new((1,), torch.float64)),
            'salsa_nn_seld_score2022': (new((n * n_seg, nc, 5), torch.int32), new((n * n_seg, nc), torch.float64), new((n * n_seg, 3), torch.int32),
                                        new((n * n_seg,), torch.int32), new((n, nc, 5), torch.int64), new((n, nc), torch.float64),
                                        new((n, 3), torch.int64))}
    ptr = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
    L = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(name):
        rc = getattr(L, name)(ptr(pr), ptr(pc), pr.shape[1], ptr(gr), ptr(gc), gr.shape[1], n, 600, 10, nc, 20.0, DEFAULT_MARGIN,
                              *[ptr(t) for t in outs[name]], stream)
        assert rc == 0, (name, rc)
    names = ('salsa_nn_seld_score', 'salsa_nn_seld_score2022')
    versions = {'salsa_nn_seld_score': '2021', 'salsa_nn_seld_score2022': '2022'}
    for _ in range(10):
        for name in names:
            call(name)
            score_dcase_rows(pr, pc, gr, gc, eval_version=versions[name])
    torch.cuda.synchronize()
    launch_ms, wall_ms = {k: [] for k in names}, {k: [] for k in names}
    for _ in range(args.samples):
        for name in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                call(name)
            e1.record()
            torch.cuda.synchronize()
            launch_ms[name].append(e0.elapsed_time(e1) / args.inner)
            t0 = time.perf_counter()
            for _ in range(args.inner):
                got = score_dcase_rows(pr, pc, gr, gc, eval_version=versions[name])
            wall_ms[name].append((time.perf_counter() - t0) * 1e3 / args.inner)
    m = SeldMetrics2022()
    for p, g in zip(pred, gt):
        m.update(p, g)
    a, b = got.file_records(), m.file_records()
    spread = lambda v: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))}     # noqa: E731
    rec = {'bench': 'seld_score2022', 'device': torch.cuda.get_device_name(0), 'files': n, 'segments': got.n_segments,
           'pred_rows': int(pc.sum()), 'gt_rows': int(gc.sum()), 'samples': args.samples, 'calls_per_sample': args.inner,
           'margin_deg': DEFAULT_MARGIN, 'n_doubt_2022': got.n_doubt, 'n_refused_2022': got.n_refused,
           'file_records_equal_2022': all((a[k] == b[k]).all() for k in b if k != 'total_DE'),
           'total_DE_max_diff_2022': float(np.abs(got.total_DE - m.total_DE).max()),
           'macro_seld_error_2022': got.seld_error(), 'macro_seld_error_host': m.seld_error()}
    for name in names:
        rec[name + '_launch_ms'] = spread(launch_ms[name])
        rec['score_dcase_rows_' + versions[name] + '_wall_ms'] = spread(wall_ms[name])
    rec['launch_median_ratio_2022_over_2021'] = rec[names[1] + '_launch_ms']['median'] / rec[names[0] + '_launch_ms']['median']
    rec['wall_median_ratio_2022_over_2021'] = rec['score_dcase_rows_2022_wall_ms']['median'] / rec['score_dcase_rows_2021_wall_ms']['median']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
