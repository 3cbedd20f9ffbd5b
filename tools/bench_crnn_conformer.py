#!/usr/bin/env python
"""Cost of the decoder's Conformer blocks.  Three legs in ONE process, timed in alternation (round r times one
call of every leg, so drift hits them alike) and reported as medians:
    n_conformer_layers 0                               the reference's network
    n_conformer_layers 2, SALSA_HIP_CONFORMER 1        the blocks on salsa_nn_res_layernorm_* / _bias_swish_dropout_* / _conv_module_*
    n_conformer_layers 2, SALSA_HIP_CONFORMER 0        every step of the blocks on torch's operators
for the bf16 training step (forward, backward, Adam) on a synthetic --batch x 7 x 640 x 200 batch (T' = 40) and the inference forward
(bf16 autocast, eval) on --batch 60-s clips (7 x 4800 x 200, T' = 300), a device synchronise around every call.  Then every new kernel
alone, forward and backward, at M = batch x 40 and batch x 300 rows of 512 (feed-forward width 1024, 7 taps, dropout 0.1; device
events around --kernel-iters back-to-back calls), next to the torch composition of the same step on the same tensors.  One JSON line
per record.

    python tools/bench_crnn_conformer.py [--rounds 20] [--warmup 3] [--infer-rounds 7] [--batch 32] [--out profiles/crnn_conformer_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

LEGS = (('n_conformer_layers=0', 0, True), ('n_conformer_layers=2 hip', 2, True), ('n_conformer_layers=2 torch', 2, False))


def _stats(prefix, t):
    import numpy as np
    t = np.array(t) * 1e3
    return {prefix + '_ms_median': round(float(np.median(t)), 3), prefix + '_ms_p10': round(float(np.percentile(t, 10)), 3),
            prefix + '_ms_p90': round(float(np.percentile(t, 90)), 3), prefix + '_ms_min': round(float(t.min()), 3),
            prefix + '_ms_max': round(float(t.max()), 3)}


def _alternate(calls, rounds, warmup):
    """calls: {leg: thunk}; -> {leg: [seconds per call]}, one call of every leg per round"""
    import torch
    from salsa_amd.crnn import conformer
    times = {k: [] for k in calls}
    for r in range(warmup + rounds):
        for name, _, hip in LEGS:
            conformer.HIP_CONFORMER = hip
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[name]()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(time.perf_counter() - t0)
    conformer.HIP_CONFORMER = True
    return times


def _event_us(fn, iters):
    import torch
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / iters * 1e3, 1)


def kernels_alone(args, dev):
    import torch
    import torch.nn as nn
    from salsa_amd.crnn import conformer
    recs = []
    for T in (40, 300):
        B, d, ff, K, p = args.batch, 512, 1024, 7, 0.1
        g = torch.Generator(device=dev).manual_seed(T)
        rand = lambda *s: torch.randn(s, device=dev, generator=g)                                # noqa: E731
        x, br, a_ff, a_cv = (rand(*s).requires_grad_(True) for s in ((B, T, d), (B, T, d), (B, T, ff), (B, T, 2 * d)))
        go, go_ff = rand(B, T, d), rand(B, T, ff)
        norm, b1 = nn.LayerNorm(d).to(dev), rand(ff).requires_grad_(True)
        dw, dwn = nn.Conv1d(d, d, K, padding=K // 2, groups=d).to(dev), nn.LayerNorm(d).to(dev)
        steps = {
            'res_layernorm': (lambda: conformer.res_layernorm(x, br, norm, 0.5, p), (x, br) + tuple(norm.parameters()), (go, go)),
            'bias_swish_dropout': (lambda: conformer.bias_swish_dropout(a_ff, b1, p), (a_ff, b1), go_ff),
            'conv_module': (lambda: conformer.conv_module_core(a_cv, dw, dwn), (a_cv,) + tuple(dw.parameters()) + tuple(dwn.parameters()), go),
        }
        rec = dict(bench='crnn_conformer_kernels', batch=B, T=T, M=B * T, d=d, ff=ff, kernel=K, dropout=p, iters=args.kernel_iters)
        for hip in (True, False):
            conformer.HIP_CONFORMER = hip
            tag = '' if hip else 'torch_'
            for name, (fwd, wrt, gout) in steps.items():
                out = fwd()
                rec[tag + name + '_fwd_us'] = _event_us(fwd, args.kernel_iters)
                rec[tag + name + '_bwd_us'] = _event_us(lambda: torch.autograd.grad(out, wrt, gout, retain_graph=True), args.kernel_iters)
        conformer.HIP_CONFORMER = True
        rec['gpu'] = torch.cuda.get_device_name(0)
        recs.append(rec)
    return recs


def run(args):
    import torch
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit('bench_crnn_conformer needs a GPU')
    dev = torch.device('cuda:0')
    x, sed, doa = synthetic_batch(args.batch, dev, seed=1)
    clips = torch.randn((args.batch, 7, 4800, 200), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    trainers = {name: Trainer(dev, total_steps=10 ** 6, n_conformer_layers=n) for name, n, _ in LEGS}
    losses = {}

    def step(name):
        losses[name] = trainers[name].train_step(x, sed, doa)[0]
    train = _alternate({name: (lambda name=name: step(name)) for name in trainers}, args.rounds, args.warmup)
    infer = _alternate({name: (lambda name=name: trainers[name].infer(clips)) for name in trainers}, args.infer_rounds, args.warmup)
    lines = []
    for name, n, hip in LEGS:
        assert bool(torch.isfinite(losses[name])), name
        med = sorted(train[name])[len(train[name]) // 2]
        lines.append(dict(bench='crnn_conformer', leg=name, n_conformer_layers=n, conformer_path=None if n == 0 else 'hip' if hip else 'torch',
                          batch=args.batch, rounds=len(train[name]), **_stats('train_step', train[name]),
                          train_chunks_per_s=round(args.batch / med, 1), infer_rounds=len(infer[name]),
                          **_stats('infer_60s_batch', infer[name]), loss=round(float(losses[name]), 5), gpu=torch.cuda.get_device_name(0)))
    del trainers
    torch.cuda.empty_cache()
    lines += kernels_alone(args, dev)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20, help='timed training steps per leg')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--infer-rounds', type=int, default=7, help='timed inference forwards per leg')
    ap.add_argument('--kernel-iters', type=int, default=50)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    run(ap.parse_args())


if __name__ == '__main__':
    main()
