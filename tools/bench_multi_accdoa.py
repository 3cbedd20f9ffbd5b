#!/usr/bin/env python
"""Times the three pieces the Multi-ACCDOA output format adds, each against its counterpart IN THE SAME PROCESS,
alternating, after a warm-up of both:

  loss    crnn.loss.adpit_loss forward + backward on (32 x 80 rows, C = 12): the fused HIP path against the float64 torch path
          (FUSED_LOSS off), with the fused accdoa_loss at (rows, 12 classes) next to them; one device-event pair per call.
  decode  32 files of 80 (a training-chunk batch) and of 600 (inference) label frames, C = 12: decode.decode_multi_rows + the copy of
          rows and counts + rows_to_list, against the copy of the float outputs + postprocess.multi_accdoa_rows per file; host clock
          around work that ends with the rows on the host.  The device launch alone is recorded too (event pair).
  step    Trainer.train_step at batch 32 (bf16, 640 x 200 chunks) with output_format 'multi_accdoa' against 'accdoa': blocks of
          --block steps, alternating, host clock around a block that ends in a device synchronise.

The median, the quartiles and the extremes are recorded.  Appends one JSON line to --out (default profiles/multi_accdoa_bench.jsonl).
No ratio is asserted: the figures are recorded as found."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quartiles(v):
    q = np.percentile(np.asarray(v, np.float64), [0, 25, 50, 75, 100])
    return {'min': q[0], 'q25': q[1], 'median': q[2], 'q75': q[3], 'max': q[4]}


def trackwise_labels(torch, batch, n_lab, C, gen):
    """slot activities that are a prefix (Bernoulli 0.05, 0.3 of those a second source, 0.3 of those a third) and unit-vector targets"""
    s0 = torch.rand(batch, n_lab, C, generator=gen) < 0.05
    s1 = s0 & (torch.rand(batch, n_lab, C, generator=gen) < 0.3)
    s2 = s1 & (torch.rand(batch, n_lab, C, generator=gen) < 0.3)
    sed = torch.cat([s0, s1, s2], dim=2).float()                                  # (B, L, 3 C)
    v = torch.randn(batch, n_lab, 3, 3 * C, generator=gen)
    v = v / v.norm(dim=2, keepdim=True)
    return sed, (v * sed[:, :, None, :]).reshape(batch, n_lab, 9 * C)


def main():
    import torch
    from salsa_amd.crnn import loss as L
    from salsa_amd.crnn.decode import decode_multi_rows, rows_to_list
    from salsa_amd.crnn.postprocess import multi_accdoa_rows
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--block', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_accdoa_bench.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this bench needs cuda:0'
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(9)
    B, n_lab, C = 32, 80, 12
    rec = {'bench': 'multi_accdoa', 'device': torch.cuda.get_device_name(0), 'batch': B, 'label_frames': n_lab, 'classes': C,
           'reps': args.reps, 'rounds': args.rounds, 'block': args.block}

    # ---------------------------------------------------------------------------------------------------------------- loss
    sed, doa_gt = (t.to(dev) for t in trackwise_labels(torch, B, n_lab, C, gen))
    pred = (0.5 * torch.randn(B, n_lab, 9 * C, generator=gen)).to(dev)
    sed1, doa1, pred1 = sed[..., :C].contiguous(), doa_gt.reshape(B, n_lab, 3, 3 * C)[..., :C].reshape(B, n_lab, 3 * C).contiguous(), \
        pred.reshape(B, n_lab, 3, 3 * C)[..., :C].reshape(B, n_lab, 3 * C).contiguous()

    def loss_call(kind):
        if kind == 'accdoa_fused':
            p, lg = pred1.clone().requires_grad_(True), torch.zeros(B, n_lab, C, device=dev, requires_grad=True)
            out = L.accdoa_loss({'event_frame_logit': lg, 'doa_frame_output': p}, sed1, doa1)[0]
        else:
            L.FUSED_LOSS = kind == 'adpit_fused'
            p, lg = pred.clone().requires_grad_(True), torch.zeros(B, n_lab, 3 * C, device=dev, requires_grad=True)
            out = L.adpit_loss({'event_frame_logit': lg, 'doa_frame_output': p}, sed, doa_gt)[0]
            L.FUSED_LOSS = True
        out.backward()
        return out
    kinds = ('adpit_fused', 'adpit_torch', 'accdoa_fused')
    for _ in range(10):
        vals = {k: float(loss_call(k).detach()) for k in kinds}
    torch.cuda.synchronize()
    events = {k: [] for k in kinds}
    for _ in range(args.reps):
        for k in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss_call(k)
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    for k in kinds:
        rec['loss_%s_ms' % k] = quartiles([a.elapsed_time(b) for a, b in events[k]])
    rec['loss_values'] = vals

    # ---------------------------------------------------------------------------------------------------------------- decode
    for frames in (80, 600):
        v = torch.randn(B, frames, 3, 3 * C, generator=gen)
        v = v / v.norm(dim=2, keepdim=True) * torch.rand(B, frames, 1, 3 * C, generator=gen)
        near = torch.rand(B, frames, 1, C, generator=gen) < 0.3                       # track 1 close to track 0 in a third of the cells
        v[..., C:2 * C] = torch.where(near, v[..., :C] + 0.05 * v[..., C:2 * C], v[..., C:2 * C])
        xyz = v.reshape(B, frames, 9 * C).to(dev)
        act = v.norm(dim=2).to(dev)

        def device_path():
            rows, counts = decode_multi_rows(act, xyz, frames, 0.5, 15.0, C)
            return rows_to_list(rows.cpu(), counts.cpu(), eval_version='2020')

        def host_path():
            a, x = act.cpu().numpy(), xyz.cpu().numpy()
            return [multi_accdoa_rows(a[f], x[f], 0.5, 15.0, C, frames, eval_version='2020') for f in range(B)]
        same = device_path() == host_path()
        wall = {'device': [], 'host': []}
        for _ in range(max(5, args.reps // 10)):
            for name, fn in (('device', device_path), ('host', host_path)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        ev = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            decode_multi_rows(act, xyz, frames, 0.5, 15.0, C)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        rec['decode_%d' % frames] = {'rows': sum(len(r) for r in out), 'rows_equal': same, 'device_wall_ms': quartiles(wall['device']),
                                     'host_wall_ms': quartiles(wall['host']), 'device_launch_ms': quartiles([a.elapsed_time(b) for a, b in ev])}

    # ---------------------------------------------------------------------------------------------------------------- step
    x, sed_a, doa_a = synthetic_batch(B, dev, seed=3)
    sed_m, doa_m = (t.to(dev) for t in trackwise_labels(torch, B, n_lab, C, gen))
    legs = {'accdoa': (Trainer(dev, total_steps=10 ** 6, output_format='accdoa'), sed_a, doa_a),
            'multi_accdoa': (Trainer(dev, total_steps=10 ** 6, output_format='multi_accdoa'), sed_m, doa_m)}
    for name, (tr, s, d) in legs.items():
        for _ in range(10):
            tr.train_step(x, s, d)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, (tr, s, d) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.block):
                tr.train_step(x, s, d)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.block)
    for name in legs:
        rec['step_%s_ms' % name] = quartiles(ms[name])
    rec['step_median_ratio_multi_over_accdoa'] = float(np.median(ms['multi_accdoa']) / np.median(ms['accdoa']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(json.dumps(rec) + '\n')
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
