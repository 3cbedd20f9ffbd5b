#!/usr/bin/env python
"""Time GpuFeatureBank.batch_augmented -- the one-call salsa_bank_batch -- against the composed path it replaces (batch(), then
augment.apply_augment_hip, then augment.swap_targets: the code as it was before the fused call existed, reached through
SALSA_BANK_BATCH=0) on a bank of the real size: 400 clips x 4800 frames x 200 bins, 7 channels (10.75 GB), seeded fill, batches of
32 chunks of 640 frames, with the MIC SALSA recipe (swaps, shifts, cutouts: the min / max launch runs) and the FOA one (no cutout).

Both paths run in ONE process and alternate batch by batch on the same indices and draws, so clock and cache state drift hits both
alike.  Per batch a pair of device events brackets the call (device time of the launches it issued); the wall time of each path's whole
run, closed by one final synchronise, gives the host-inclusive time per batch.  Medians and quartiles over --batches batches after
--warmup go to profiles/bank_batch_bench.jsonl, one JSON line per recipe.

    python tools/bench_bank_batch.py [--batches 200] [--warmup 20] [--clips 400]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_bank(n_clips, n_frames, F, seed):
    """the bank's fields filled directly on the device (no files): seeded features, sparse labels, the reference's chunk indices"""
    from salsa_amd.dataset import GpuFeatureBank, get_segment_idxes
    bank = GpuFeatureBank(None, device='cuda')
    g = torch.Generator(device='cuda').manual_seed(seed)
    feats = torch.empty((7, n_clips * n_frames, F), device='cuda')
    for c in range(7):                                                        # (channel by channel: no second 10-GB temporary)
        feats[c].normal_(generator=g)
    bank.features = feats
    n_lab = n_clips * n_frames // bank.upsample
    bank.sed_all = (torch.rand((n_lab, 12), device='cuda', generator=g) < 0.05).float()
    bank.doa_all = torch.randn((n_lab, 36), device='cuda', generator=g) * bank.sed_all.repeat(1, 3)
    for i in range(n_clips):
        idx, bank.pointer = get_segment_idxes(n_frames, bank.chunk_len, bank.chunk_hop_len, 1, bank.pointer)
        gidx, bank.gt_pointer = get_segment_idxes(n_frames, bank.chunk_len, bank.chunk_hop_len, bank.upsample, bank.gt_pointer)
        bank.chunk_idx += idx
        bank.gt_idx += gidx
        bank.chunk_name += ['clip%03d' % i] * len(idx)
    return bank


def quartiles(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return dict(q25=round(float(q[0]), 4), median=round(float(q[1]), 4), q75=round(float(q[2]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--clips', type=int, default=400)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bank_batch_bench.jsonl'))
    args = ap.parse_args()
    from salsa_amd.dataset import BankLoader
    bank = build_bank(args.clips, 4800, 200, seed=0)
    torch.cuda.synchronize()
    lines = []
    for fmt in ('mic', 'foa'):
        loader = BankLoader(bank, batch_size=args.batch_size, seed=1, audio_format=fmt)
        n = args.warmup + args.batches
        assert len(loader) >= n, 'the bank has %d batches per epoch, %d wanted' % (len(loader), n)
        work = [(loader.step_indices(0, s).tolist(), loader.step_draws(0, s, args.batch_size)) for s in range(n)]   # draws made once, outside the clock
        ev = {p: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)] for p in ('fused', 'composed')}
        host = {'fused': 0.0, 'composed': 0.0}
        for s, (idx, d) in enumerate(work):
            for path in (('fused', 'composed') if s % 2 == 0 else ('composed', 'fused')):   # alternate, and alternate who goes first
                os.environ['SALSA_BANK_BATCH'] = '1' if path == 'fused' else '0'
                t0 = time.perf_counter()
                ev[path][s][0].record()
                out = bank.batch_augmented(idx, d, fmt, 'salsa')
                ev[path][s][1].record()
                if s >= args.warmup:
                    host[path] += time.perf_counter() - t0                    # host time to ISSUE the batch (no synchronise inside)
                del out
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                              # the one synchronise
        drain = time.perf_counter() - t0
        os.environ.pop('SALSA_BANK_BATCH', None)
        rec = dict(bench='bank_batch', device=torch.cuda.get_device_name(0), recipe=fmt, clips=args.clips, bank_gb=round(bank.features.numel() * 4 / 1e9, 2),
                   batch=args.batch_size, chunk_frames=bank.chunk_len, batches=args.batches, warmup=args.warmup, drain_ms=round(drain * 1e3, 3))
        for path in ('fused', 'composed'):
            ms = [a.elapsed_time(b) for a, b in ev[path][args.warmup:]]
            rec[path + '_device_ms'] = quartiles(ms)
            rec[path + '_host_issue_ms'] = round(host[path] / args.batches * 1e3, 4)
        rec['device_median_ratio_composed_over_fused'] = round(rec['composed_device_ms']['median'] / rec['fused_device_ms']['median'], 3)
        lines.append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for rec in lines:
            f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
