#!/usr/bin/env python
"""Cost of the decoder's self-attention stage.  Three legs in ONE process, timed in alternation (round r times
one call of every leg, so drift hits them alike) and reported as medians:
    n_attn_layers 0                              the reference's network
    n_attn_layers 2, SALSA_HIP_ATTN 1            the blocks on salsa_nn_attn_* / salsa_nn_add_layernorm_*
    n_attn_layers 2, SALSA_HIP_ATTN 0            the blocks on nn.MultiheadAttention / F.layer_norm
for the bf16 training step (forward, backward, Adam) on a synthetic --batch x 7 x 640 x 200 batch (T' = 40) and the inference forward
(bf16 autocast, eval) on --batch 60-s clips (7 x 4800 x 200, T' = 300), a device synchronise around every call.  Then the two
kernels alone at both shapes (8 heads of 64; device events around --kernel-iters back-to-back launches), next to torch's own
operators on the same tensors (F.scaled_dot_product_attention and F.layer_norm(x + res), float32).  One JSON line per record.

    python tools/bench_crnn_attn.py [--rounds 20] [--warmup 3] [--infer-rounds 7] [--batch 32] [--out profiles/crnn_attn_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

LEGS = (('n_attn_layers=0', 0, True), ('n_attn_layers=2 hip', 2, True), ('n_attn_layers=2 torch', 2, False))


def _stats(prefix, t):
    import numpy as np
    t = np.array(t) * 1e3
    return {prefix + '_ms_median': round(float(np.median(t)), 3), prefix + '_ms_p10': round(float(np.percentile(t, 10)), 3),
            prefix + '_ms_p90': round(float(np.percentile(t, 90)), 3), prefix + '_ms_min': round(float(t.min()), 3),
            prefix + '_ms_max': round(float(t.max()), 3)}


def _alternate(calls, rounds, warmup):
    """calls: {leg: thunk}; -> {leg: [seconds per call]}, one call of every leg per round"""
    import torch
    from salsa_amd.crnn import attention
    times = {k: [] for k in calls}
    for r in range(warmup + rounds):
        for name, _, hip in LEGS:
            attention.HIP_ATTN = hip
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls[name]()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(time.perf_counter() - t0)
    attention.HIP_ATTN = True
    return times


def _event_ms(fn, iters):
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
    return a.elapsed_time(b) / iters


def kernels_alone(args, dev):
    import torch
    import torch.nn.functional as F
    from salsa_amd.crnn.attention import add_layernorm, attn_core
    recs = []
    for T in (40, 300):
        B, H, dh = args.batch, 8, 64
        d = H * dh
        g = torch.Generator(device=dev).manual_seed(T)
        qkv = torch.randn((B, T, 3 * d), device=dev, generator=g, requires_grad=True)
        go = torch.randn((B, T, d), device=dev, generator=g)
        out = attn_core(qkv, H)
        q, k, v = (t.transpose(1, 2) for t in qkv.detach().view(B, T, 3, H, dh).unbind(2))   # (B, H, T, dh) views
        q, k, v = (t.contiguous().requires_grad_(True) for t in (q, k, v))
        so = F.scaled_dot_product_attention(q, k, v)
        sgo = go.view(B, T, H, dh).transpose(1, 2).contiguous()
        x = torch.randn((B, T, d), device=dev, generator=g, requires_grad=True)
        res = torch.randn((B, T, d), device=dev, generator=g, requires_grad=True)
        w = torch.ones(d, device=dev, requires_grad=True)
        b = torch.zeros(d, device=dev, requires_grad=True)
        y, ty = add_layernorm(x, res, w, b, 1e-5), F.layer_norm(x + res, (d,), w, b, 1e-5)
        rec = dict(bench='crnn_attn_kernels', batch=B, T=T, n_heads=H, head_dim=dh, iters=args.kernel_iters,
                   attn_fwd_us=_event_ms(lambda: attn_core(qkv, H), args.kernel_iters) * 1e3,
                   attn_bwd_us=_event_ms(lambda: torch.autograd.grad(out, qkv, go, retain_graph=True), args.kernel_iters) * 1e3,
                   torch_sdpa_fwd_us=_event_ms(lambda: F.scaled_dot_product_attention(q, k, v), args.kernel_iters) * 1e3,
                   torch_sdpa_bwd_us=_event_ms(lambda: torch.autograd.grad(so, (q, k, v), sgo, retain_graph=True), args.kernel_iters) * 1e3,
                   add_layernorm_fwd_us=_event_ms(lambda: add_layernorm(x, res, w, b, 1e-5), args.kernel_iters) * 1e3,
                   add_layernorm_bwd_us=_event_ms(lambda: torch.autograd.grad(y, (x, res, w, b), go, retain_graph=True), args.kernel_iters) * 1e3,
                   torch_add_layernorm_fwd_us=_event_ms(lambda: F.layer_norm(x + res, (d,), w, b, 1e-5), args.kernel_iters) * 1e3,
                   torch_add_layernorm_bwd_us=_event_ms(lambda: torch.autograd.grad(ty, (x, res, w, b), go, retain_graph=True),
                                                        args.kernel_iters) * 1e3,
                   gpu=torch.cuda.get_device_name(0))
        recs.append({k: (round(v, 1) if isinstance(v, float) else v) for k, v in rec.items()})
    return recs


def run(args):
    import torch
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit('bench_crnn_attn needs a GPU')
    dev = torch.device('cuda:0')
    x, sed, doa = synthetic_batch(args.batch, dev, seed=1)
    clips = torch.randn((args.batch, 7, 4800, 200), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    trainers = {name: Trainer(dev, total_steps=10 ** 6, n_attn_layers=n) for name, n, _ in LEGS}
    losses = {}

    def step(name):
        losses[name] = trainers[name].train_step(x, sed, doa)[0]
    train = _alternate({name: (lambda name=name: step(name)) for name in trainers}, args.rounds, args.warmup)
    infer = _alternate({name: (lambda name=name: trainers[name].infer(clips)) for name in trainers}, args.infer_rounds, args.warmup)
    lines = []
    for name, n, hip in LEGS:
        assert bool(torch.isfinite(losses[name])), name
        med = sorted(train[name])[len(train[name]) // 2]
        lines.append(dict(bench='crnn_attn', leg=name, n_attn_layers=n, attn_path=None if n == 0 else 'hip' if hip else 'torch',
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
