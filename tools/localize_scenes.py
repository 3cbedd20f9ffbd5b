#!/usr/bin/env python
"""What the features' directional channels say about rendered scenes, without a network: draw_scenes at
polyphony 1 and 2, render, extract, DoaHistogram.localize, angular_errors against the scenes' own rows.  Responses: make_rir_bank
anechoic and with rt60 = 0.3 s, room_rir_bank in a 6 x 5 x 3.2 m shoebox (nominal rt60 0.3 s) -- FOA, MIC open, MIC rigid each -- with a
white ambient of 0.001 alone and with a DiffuseField at 20 dB SNR on top.  Per case: median and 95th percentile of the matched peaks'
angular error, missed and extra peaks per label frame, peaks per frame.  ONE run each: records, not claims.  A frame in which an event
starts or ends counts like any other, so the missed and extra figures include the onsets' and decays' frames.

    python tools/localize_scenes.py [--clips 8] [--seconds 20] [--out profiles/doa_hist_scenes.jsonl]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=8)
    ap.add_argument('--seconds', type=int, default=20)
    ap.add_argument('--rir-len', type=int, default=7200)
    ap.add_argument('--distance', type=float, default=1.5)
    ap.add_argument('--snr-db', type=float, default=20.0)
    ap.add_argument('--seed', type=int, default=2021)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import localize as lz, scenes as sc
    from salsa_amd.extractor import SalsaExtractor
    dev = torch.device('cuda:0')
    B, n = args.clips, args.seconds * sc.FS
    pool = sc.synth_event_pool(12, 4, 0)
    directions = [(a, e) for a in range(-180, 180, 30) for e in (-40, -10, 20, 50)]
    room = sc.ShoeboxRoom((6.0, 5.0, 3.2), rt60=0.3)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    for fmt, baffle in (('foa', 'open'), ('mic', 'open'), ('mic', 'rigid')):
        kw = dict(baffle=baffle) if fmt == 'mic' else {}
        fmax = 9000 if fmt == 'foa' else 4000
        ex = SalsaExtractor(audio_format=fmt, fmax_doa=fmax, device=dev)
        loc = lz.DoaHistogram(audio_format=fmt, fmax_doa=fmax)
        field = sc.DiffuseField(fmt, **kw)
        banks = (('make_rir_bank anechoic', lambda: sc.make_rir_bank(fmt, directions, 128, **kw)),
                 ('make_rir_bank rt60 0.3', lambda: sc.make_rir_bank(fmt, directions, args.rir_len, rt60=0.3, seed=1, **kw)),
                 ('room_rir_bank 6x5x3.2 nominal rt60 0.3', lambda: sc.room_rir_bank(fmt, room, directions, args.distance, args.rir_len, device=dev, **kw)))
        for bank_name, make in banks:
            bank = make()
            for polyphony in (1, 2):
                scenes = sc.draw_scenes(B, pool, bank, n, args.seed, max_polyphony=polyphony)
                g = torch.Generator(dev).manual_seed(args.seed)
                ambient = 1e-3 * torch.randn((B, 4, n), device=dev, generator=g)
                clean = sc.render_scenes(scenes, pool, bank, ambient=ambient)
                for diffuse in (False, True):
                    audio = clean.clone()
                    if diffuse:
                        sc.add_diffuse(audio, field, snr_db=args.snr_db, seeds=args.seed, out=audio)
                    res = loc.localize(ex.extract(audio))
                    e = lz.angular_errors(res, scenes)
                    r = res.numpy()
                    rows = sum(int((sc.scene_rows(scenes[b])[:, 0] < r.count.shape[1]).sum()) for b in range(B))
                    emit(dict(record='doa_hist_scenes', array='%s %s' % (fmt, baffle), responses=bank_name, polyphony=polyphony,
                              diffuse_snr_db=args.snr_db if diffuse else None, clips=B, seconds=args.seconds, label_frames=e.n_frames,
                              ground_truth_rows=rows, matched=len(e.errors),
                              error_deg_median=round(float(np.median(e.errors)), 2) if len(e.errors) else None,
                              error_deg_p95=round(float(np.percentile(e.errors, 95)), 2) if len(e.errors) else None,
                              missed_per_frame=round(e.missed / e.n_frames, 4), extra_per_frame=round(e.extra / e.n_frames, 4),
                              peaks_per_frame=round(float(r.count.mean()), 4), votes_per_frame_mean=round(float(r.n_votes.mean()), 1),
                              columns=[loc.col0, loc.col1], grid_step=loc.grid_step, max_sources=loc.max_sources, runs=1,
                              device=torch.cuda.get_device_name(0)))
                del clean, ambient


if __name__ == '__main__':
    main()
