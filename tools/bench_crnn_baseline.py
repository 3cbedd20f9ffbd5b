#!/usr/bin/env python
"""Training-step throughput of the SELD CRNN on the baseline features (melspeciv / linspeciv: 7 channels, melspecgcc /
linspecgcc: 10; 128 mel or 200 linear bins): one bf16 Trainer step (forward, backward, Adam) on a synthetic batch of
--batch x --frames chunks, timed with a device synchronise around each step.  For the GCC types the same step also runs with
the first layer on MIOpen (SALSA_HIP_STEM16=0), alternated with the HIP path in blocks inside this one process.  One JSON line
per (feature type, first-layer path): chunks/s and the step-time median / 10th / 90th percentile / min / max.

    python tools/bench_crnn_baseline.py [--steps 24] [--warmup 4] [--types melspecgcc,linspecgcc] [--out FILE]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_crnn_baseline.py --steps 4`."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

TYPES = {'melspeciv': (7, 128), 'linspeciv': (7, 200), 'melspecgcc': (10, 128), 'linspecgcc': (10, 200)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=24, help='timed steps per (type, path)')
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=640)
    ap.add_argument('--types', default=','.join(TYPES))
    ap.add_argument('--block', type=int, default=4, help='steps per block when two paths alternate')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()

    import numpy as np
    import torch
    from salsa_amd.crnn import nn_ops
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit('bench_crnn_baseline needs a GPU')
    dev = torch.device('cuda:0')
    lines = []
    for ft in args.types.split(','):
        cin, nf = TYPES[ft]
        tr = Trainer(dev, total_steps=10 ** 6, n_input_channels=cin)
        x, sed, doa = synthetic_batch(args.batch, dev, seed=1, n_frames=args.frames, n_freq=nf, n_channels=cin)
        paths = [True, False] if cin > 8 else [True]
        for on in paths:                                          # warm-up: every path the timed window uses
            nn_ops.USE_HIP_STEM16 = on
            for _ in range(args.warmup):
                tr.train_step(x, sed, doa)
        torch.cuda.synchronize()
        times = {on: [] for on in paths}
        while min(len(v) for v in times.values()) < args.steps:
            for on in paths:
                nn_ops.USE_HIP_STEM16 = on
                for _ in range(min(args.block, args.steps - len(times[on]))):
                    t0 = time.perf_counter()
                    loss = tr.train_step(x, sed, doa)[0]
                    torch.cuda.synchronize()
                    times[on].append(time.perf_counter() - t0)
        nn_ops.USE_HIP_STEM16 = True
        assert bool(torch.isfinite(loss))
        for on in paths:
            t = np.array(times[on]) * 1e3
            rec = dict(bench='crnn_baseline_train_step', feature_type=ft, n_input_channels=cin, n_freq=nf, batch=args.batch,
                       frames=args.frames, first_layer='hip_stem16' if (on and cin > 8) else ('hip_stem' if on else 'miopen'),
                       steps=len(t), chunks_per_s=round(args.batch / (float(np.median(t)) / 1e3), 1),
                       step_ms_median=round(float(np.median(t)), 3), step_ms_p10=round(float(np.percentile(t, 10)), 3),
                       step_ms_p90=round(float(np.percentile(t, 90)), 3), step_ms_min=round(float(t.min()), 3),
                       step_ms_max=round(float(t.max()), 3), gpu=torch.cuda.get_device_name(0))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del tr, x, sed, doa
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
