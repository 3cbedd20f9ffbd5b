#!/usr/bin/env python
"""Times of the config-5 inference forward (bf16 autocast, eval) on --batch 60-s clips (7 x 4800 x 200) under test-time augmentation
and ensembling, all legs in ONE process and interleaved (every round times each leg once, so drift of the
shared host hits all legs alike); each call is timed by a host clock around the call and a device synchronise:

    plain           Trainer.infer
    tta16_foa       TtaForward, the 16 FOA variants               tta16_foa_torch   the same with SALSA_HIP_TTA=0's torch operators
    tta8_mic        TtaForward, the 8 MIC variants                tta8_mic_torch
    ensemble2       two models, identity only                     ensemble2_torch
    variant_only    one salsa_nn_tta_variant launch on the clips (FOA variant 15, MIC variant 7)
    merge_only      one salsa_nn_tta_merge launch on 16 slabs

One JSON line per leg: median / 10th / 90th percentile / min / max in ms, the number of forwards N, the leg's time over N x the plain
median of the same process, and the overhead in percent.

    python tools/bench_crnn_tta.py [--steps 10] [--warmup 2] [--batch 32] [--out profiles/crnn_tta_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def _stats(t):
    import numpy as np
    t = np.array(t) * 1e3
    return dict(ms_median=round(float(np.median(t)), 3), ms_p10=round(float(np.percentile(t, 10)), 3),
                ms_p90=round(float(np.percentile(t, 90)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10, help='timed rounds (every leg once per round)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=4800, help='feature frames per clip (4800 = 60 s)')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import torch
    from salsa_amd.crnn import tta
    from salsa_amd.crnn.train import Trainer
    if not torch.cuda.is_available():
        raise SystemExit('bench_crnn_tta needs a GPU')
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(5)
    clips = torch.randn((args.batch, 7, args.frames, 200), device=dev, generator=g)
    tr, tr2 = Trainer(dev, total_steps=10 ** 6), Trainer(dev, total_steps=10 ** 6)
    wrapped = dict(tta16_foa=tta.TtaForward(tr.infer, 'foa', 'salsa'), tta8_mic=tta.TtaForward(tr.infer, 'mic', 'salsa'),
                   ensemble2=tta.TtaForward([tr.infer, tr2.infer], 'foa', 'salsa', variants=None))
    n_forwards = dict(plain=1, tta16_foa=16, tta8_mic=8, ensemble2=2)
    L = tr.infer(clips[:1])[0].shape[1]
    slabs = (torch.rand((16, args.batch, L, 12), device=dev), torch.rand((16, args.batch, L, 36), device=dev))
    scratch = torch.empty_like(clips)

    def with_switch(on, f):
        def call():
            tta.USE_HIP_TTA = on
            try:
                return f()
            finally:
                tta.USE_HIP_TTA = True
        return call

    legs = {'plain': lambda: tr.infer(clips)}
    for name, w in wrapped.items():
        legs[name] = with_switch(True, lambda w=w: w(clips))
        legs[name + '_torch'] = with_switch(False, lambda w=w: w(clips))
    legs['variant_only_foa15'] = lambda: tta.tta_variant(clips, 'foa', 15, out=scratch)
    legs['variant_only_mic7'] = lambda: tta.tta_variant(clips, 'mic', 7, out=scratch)
    legs['merge_only_16'] = lambda: tta.tta_merge(slabs[0], slabs[1], 1, list(range(16)), 'foa', 12)
    times = {name: [] for name in legs}
    for step in range(args.warmup + args.steps):
        for name, f in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = f()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times[name].append(time.perf_counter() - t0)
            del out
    plain = _stats(times['plain'])['ms_median']
    lines = []
    for name, t in times.items():
        rec = dict(bench='crnn_tta', leg=name, batch=args.batch, frames=args.frames, calls=len(t), **_stats(t))
        n = n_forwards.get(name.replace('_torch', ''))
        if n:
            rec.update(forwards=n, plain_ms_median=plain, over_n_plain=round(rec['ms_median'] / (n * plain), 4),
                       overhead_pct=round(100.0 * (rec['ms_median'] / (n * plain) - 1.0), 2))
        rec['gpu'] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
