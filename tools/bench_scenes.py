#!/usr/bin/env python
"""Time of the scene renderer.  Two legs in ONE process, one call of each per round so that drift hits them alike,
medians after warm-up, device events around each call between two synchronises:
    hip          render_scenes on salsa_scene_render (salsa_amd/csrc/scene_render.hip)
    torch.fft    the same definition composed from torch.fft calls, one per item (SALSA_HIP_SCENE=0)
(each timed sample is --calls back-to-back calls of one leg, reported per call) at two sizes: --batch clips of 60 s with about 30 items each at a response of 7200 taps, and --batch clips of 8 s (the chunk length
of BASELINE config 4).  Both legs include their table uploads and allocations: a call is what a user's call costs.  The algorithmic
flops and bytes are computed from the shapes, here, and the rates are those of the whole call, not of a kernel.  The two legs' outputs
are compared at the sizes that are timed.  One JSON line per record; whatever is seen is reported, slower included.

    python tools/bench_scenes.py [--rounds 9] [--calls 5] [--warmup 2] [--batch 32] [--out profiles/scene_render_bench.jsonl]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

PART = 512


def work(scenes, pool, bank):
    """the algorithmic work of one render, from the shapes: direct-form MACs of the definition, and what the partitioned overlap-save
    does -- transforms (5 n log2 n flops for a complex transform of n = 512, forward or inverse), spectrum MACs (8 flops per complex
    multiply-add), and the bytes its launches move (spectra read per (output block, item, partition), workspace written and read)."""
    import numpy as np
    N, C, L = scenes.n_samples, bank.n_channels, bank.length
    P, M = -(-L // PART), -(-N // PART)
    ln = pool.lengths[scenes.event]
    direct_macs = int(np.sum(ln * L) * C)
    j0 = scenes.onset // PART
    j1 = np.minimum((scenes.onset + ln - 1) // PART + 1, M - 1)
    item_ffts = int(np.sum(j1 - j0 + 1))
    pairs, active = 0, 0
    for b in range(scenes.n_clips):
        sl = slice(scenes.clip_start[b], scenes.clip_start[b + 1])
        cover = np.zeros(M, np.int64)
        for a, z in zip(j0[sl], j1[sl]):
            for p in range(P):                                                 # output block m = j + p for every input block j of the item
                lo, hi = a + p, min(z + p, M - 1)
                if lo <= hi:
                    cover[lo:hi + 1] += 1
        pairs += int(cover.sum())
        active += int((cover > 0).sum())
    fft_flops = 5 * PART * 9
    flops = item_ffts * fft_flops + active * C * fft_flops + pairs * C * PART * 8
    moved = item_ffts * PART * 8 + pairs * (1 + C) * PART * 8 + 2 * scenes.n_clips * C * N * 4
    return dict(items=int(scenes.n_items), direct_form_gmac=round(direct_macs / 1e9, 3), ols_gflop=round(flops / 1e9, 3),
                item_transforms=item_ffts, output_blocks_rendered=active, output_blocks=int(scenes.n_clips * M), spectrum_pairs=pairs,
                ols_gbytes=round(moved / 1e9, 3), audio_gbytes=round(2 * scenes.n_clips * C * N * 4 / 1e9, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--calls', type=int, default=5, help='back-to-back calls per timed sample')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rir-len', type=int, default=7200)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import scenes as sc
    dev = torch.device('cuda:0')
    pool = sc.synth_event_pool(12, 4, 0, min_s=1.0, max_s=3.0)
    bank = sc.make_rir_bank('foa', [(a, e) for a in range(-180, 180, 30) for e in (-30, 0, 30)], args.rir_len, rt60=0.3, seed=1)
    bank.spectra(dev)                                                          # once per bank: not part of a render
    recs = []
    for tag, seconds in (('60 s', 60), ('8 s', 8)):
        n = seconds * sc.FS
        scenes = sc.draw_scenes(args.batch, pool, bank, n, 2021)
        amb = 1e-3 * torch.randn(args.batch, 4, n, device=dev)
        out = torch.empty_like(amb)
        times = {'hip': [], 'torch.fft': []}
        peak = {}
        for r in range(args.warmup + args.rounds):
            for leg in times:
                sc.HIP_SCENE = leg == 'hip'
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                a.record()
                for _ in range(args.calls):
                    sc.render_scenes(scenes, pool, bank, ambient=amb, out=out)
                b.record()
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                if r >= args.warmup:
                    times[leg].append(a.elapsed_time(b) / args.calls)
        sc.HIP_SCENE = False
        other = sc.render_scenes(scenes, pool, bank, ambient=amb)
        sc.HIP_SCENE = True
        sc.render_scenes(scenes, pool, bank, ambient=amb, out=out)
        diff, top = float((out - other).abs().max()), float(other.abs().max())
        del other
        w = work(scenes, pool, bank)
        w.update(max_abs_difference_of_the_legs=diff, max_abs_output=round(top, 4))
        for leg, t in times.items():
            t = np.array(t)
            rec = dict(bench='scene_render', size='%d x %s' % (args.batch, tag), leg=leg, rir_len=args.rir_len, n_samples=n,
                       ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
                       rounds=len(t), calls_per_sample=args.calls, temporaries_mb=round(peak[leg] / 2 ** 20, 1), device=torch.cuda.get_device_name(0), **w)
            if leg == 'hip':
                rec['call_ols_gflop_per_s'] = round(w['ols_gflop'] / (np.median(t) * 1e-3), 1)
                rec['call_ols_gbyte_per_s'] = round(w['ols_gbytes'] / (np.median(t) * 1e-3), 1)
            recs.append(rec)
        recs.append(dict(bench='scene_render', size='%d x %s' % (args.batch, tag), hip_over_torch_fft=round(
            float(np.median(times['hip']) / np.median(times['torch.fft'])), 3)))
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
