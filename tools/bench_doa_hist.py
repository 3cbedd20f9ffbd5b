#!/usr/bin/env python
"""Time of the DOA histogram.  Two legs in ONE process, alternating round by round so that drift hits them alike,
medians after warm-up, device events around whole calls between two synchronises:
    hip      DoaHistogram.localize on salsa_doa_hist (salsa_amd/csrc/doa_hist.hip), and the launch alone on resident outputs
    torch    the same definition composed from torch calls on the device (SALSA_HIP_DOA=0)
Workload: --batch clips of --seconds s of RENDERED scenes (draw_scenes on make_rir_bank responses, white ambient of 0.001) through
SalsaExtractor: FOA (7, 4801, 200) with the columns [0, 191), MIC with [0, 33); 5-degree grid, K = 2.  The votes per label frame are
read from the result; the fused multiply-adds are counted from the shapes: 3 per (vote, grid cell) for the dot products of the score --
once with the votes cast and once with every cell of the window voting.  The two legs' results are compared at the size that is timed.
One JSON line per record; whatever is seen is reported, slower included.

    python tools/bench_doa_hist.py [--rounds 7] [--warmup 1] [--torch-rounds 7] [--batch 32] [--seconds 60] [--out profiles/doa_hist_bench.jsonl]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--torch-rounds', type=int, default=7, help='timed rounds of the torch leg (0: the leg is left out)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seconds', type=int, default=60)
    ap.add_argument('--grid-step', type=int, default=5)
    ap.add_argument('--sources', type=int, default=2)
    ap.add_argument('--formats', nargs='+', default=['foa', 'mic'])
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import localize as lz, scenes as sc
    from salsa_amd.extractor import SalsaExtractor
    dev = torch.device('cuda:0')
    B, n = args.batch, args.seconds * sc.FS

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    pool = sc.synth_event_pool(12, 4, 0)
    directions = [(a, e) for a in range(-180, 180, 30) for e in (-40, -10, 20, 50)]
    for fmt in args.formats:
        fmax = 9000 if fmt == 'foa' else 4000
        bank = sc.make_rir_bank(fmt, directions, 64)
        scenes = sc.draw_scenes(B, pool, bank, n, 2021)
        feats = []
        ex = SalsaExtractor(audio_format=fmt, fmax_doa=fmax, device=dev)
        g = torch.Generator(dev).manual_seed(7)
        for lo in range(0, B, 8):
            hi = min(B, lo + 8)
            ambient = 1e-3 * torch.randn((hi - lo, 4, n), device=dev, generator=g)
            feats.append(ex.extract(sc.render_scenes(scenes.clips(lo, hi), pool, bank, ambient=ambient)))
        x = torch.cat(feats)
        del feats, ambient
        loc = lz.DoaHistogram(audio_format=fmt, fmax_doa=fmax, grid_step=args.grid_step, max_sources=args.sources)
        lz.HIP_DOA = True
        res = loc.localize(x)

        def call():
            return loc.localize(x)

        def launch():
            loc.launch(x, res)

        times = {'hip call': [], 'hip launch': [], 'torch call': []}
        for r in range(args.warmup + max(args.rounds, args.torch_rounds)):
            lz.HIP_DOA = True
            for leg, fn in (('hip call', call), ('hip launch', launch)):
                t = timed(fn)
                if args.warmup <= r < args.warmup + args.rounds:
                    times[leg].append(t)
            if args.torch_rounds and r < args.warmup + args.torch_rounds:
                lz.HIP_DOA = False
                t = timed(call)
                if r >= args.warmup:
                    times['torch call'].append(t)
        lz.HIP_DOA = True
        hip = loc.localize(x).numpy()
        compare = {}
        if args.torch_rounds:
            lz.HIP_DOA = False
            other = loc.localize(x).numpy()
            lz.HIP_DOA = True
            same = (hip.count == other.count) & np.all(hip.cell == other.cell, axis=-1)
            compare = dict(frames_with_equal_decisions=int(same.sum()), frames=int(same.size),
                           max_abs_score_difference_there=float(np.abs(hip.score - other.score)[same].max()),
                           max_abs_direction_difference_there=float(np.abs(hip.direction - other.direction)[same].max()))
        Fl, G, cells = hip.count.shape[1], loc.n_cells, loc.frames_per_label * (loc.col1 - loc.col0)
        votes = hip.n_votes.astype(np.int64)
        w = dict(label_frames=int(B * Fl), grid_cells=G, window_cells=cells, votes_per_frame_mean=round(float(votes.mean()), 1),
                 votes_per_frame_max=int(votes.max()), frames_without_votes=int((votes == 0).sum()), peaks=int(hip.count.sum()),
                 gfma_of_the_votes_cast=round(3.0 * votes.sum() * G / 1e9, 3), gfma_if_every_cell_voted=round(3.0 * B * Fl * cells * G / 1e9, 3),
                 feature_gbytes_read=round(3.0 * B * Fl * cells * 4 / 1e9, 4), **compare)
        for leg, t in times.items():
            if not t:
                continue
            t = np.array(t)
            rec = dict(bench='doa_hist', format=fmt, shape=list(x.shape), columns=[loc.col0, loc.col1], grid_step=args.grid_step,
                       max_sources=args.sources, leg=leg, ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3),
                       ms_max=round(float(t.max()), 3), samples=len(t), device=torch.cuda.get_device_name(0), **w)
            if leg == 'hip launch':
                rec['launch_gfma_per_s_of_the_votes_cast'] = round(w['gfma_of_the_votes_cast'] / (np.median(t) * 1e-3), 1)
            emit(rec)
        if times['torch call']:
            emit(dict(bench='doa_hist', format=fmt, hip_call_over_torch_call=round(float(np.median(times['hip call']) / np.median(times['torch call'])), 5)))
        del x, res


if __name__ == '__main__':
    main()
