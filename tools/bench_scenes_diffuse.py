#!/usr/bin/env python
"""Time of the diffuse ambient noise.  Two legs in ONE process, alternating round by round so that drift hits
them alike, medians after warm-up, device events around each timed sample between two synchronises:
    hip      add_diffuse on salsa_scene_diffuse (salsa_amd/csrc/scene_diffuse.hip)
    torch    the same definition composed from torch calls on the device (SALSA_HIP_SCENE=0): the hash in int64 tensor arithmetic, conv1d
Whole calls (the level's scale computed on the device, the seeds uploaded: what a user's call costs), and for the hip leg the launch
alone through the C ABI on resident arguments.  Shapes: --batch clips of 60 s and of 8 s; FOA (1 mix tap), MIC open and MIC rigid (the
taps their fields have); 64 directions; 'room' colour.  The torch leg walks the clips 65536 samples at a time and is timed over
--torch-rounds rounds of ONE call.  The algorithmic work is computed from the shapes, and the rate is that of the launch.  The two legs'
outputs are compared at the sizes that are timed.  One JSON line per record; whatever is seen is reported, slower included.

    python tools/bench_scenes_diffuse.py [--rounds 7] [--calls 3] [--warmup 1] [--torch-rounds 2] [--batch 32] [--out profiles/scene_diffuse_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3, help='back-to-back hip calls per timed sample')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--torch-rounds', type=int, default=2, help='timed rounds of the torch leg, one call each (0: the leg is left out)')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--directions', type=int, default=64)
    ap.add_argument('--seconds', type=int, nargs='+', default=[60, 8])
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import _lib, ambient as amb, scenes as sc
    dev = torch.device('cuda:0')
    L = _lib.load()
    B = args.batch

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    for fmt, baffle in (('foa', 'open'), ('mic', 'open'), ('mic', 'rigid')):
        field = amb.DiffuseField(fmt, baffle=baffle, n_directions=args.directions, colour='room')
        D, La, Lg = field.n_directions, field.mix_taps, field.colour_taps
        mix, colour = field.on(dev)
        for seconds in args.seconds:
            n = seconds * sc.FS
            audio = 0.05 * torch.randn(B, 4, n, device=dev)
            out = torch.empty_like(audio)
            seeds = amb._seeds_on(2021, B, dev)
            scales = torch.full((B,), float(field.scale_for(-40.0)), dtype=torch.float32, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ptr = lambda t: C.c_void_p(t.data_ptr())

            def launch():
                rc = L.salsa_scene_diffuse(ptr(mix), D, 4, La, ptr(colour), Lg, ptr(seeds), ptr(scales), ptr(audio), ptr(out), B, n, stream)
                assert rc == 0, _lib.last_error()

            def call():
                amb.add_diffuse(audio, field, snr_db=20.0, seeds=2021, out=out)

            times = {'hip call': [], 'hip launch': [], 'torch call': []}
            for r in range(args.warmup + args.rounds):
                sc.HIP_SCENE = True
                for leg, fn in (('hip call', call), ('hip launch', launch)):
                    t = timed(fn, args.calls)
                    if r >= args.warmup:
                        times[leg].append(t)
                if r < args.torch_rounds + min(1, args.warmup) and args.torch_rounds:
                    sc.HIP_SCENE = False
                    t = timed(call, 1)
                    if r >= min(1, args.warmup):
                        times['torch call'].append(t)
            diff = top = None
            if args.torch_rounds:
                sc.HIP_SCENE = False
                other = amb.add_diffuse(audio, field, snr_db=20.0, seeds=2021, out=torch.empty_like(audio))
                sc.HIP_SCENE = True
                call()
                diff, top = float((out - other).abs().max()), float((other - audio).abs().max())
                del other
            sc.HIP_SCENE = True
            samples = B * n
            fma = samples * (4 * D * La + 4 * Lg)
            w = dict(samples=samples, gfma=round(fma / 1e9, 2), ghash=round(samples * D / 1e9, 3), audio_gbytes=round(2 * samples * 4 * 4 / 1e9, 3),
                     max_abs_difference_of_the_legs=diff, max_abs_noise=top)
            for leg, t in times.items():
                if not t:
                    continue
                t = np.array(t)
                rec = dict(bench='scene_diffuse', array='%s %s' % (fmt, baffle), size='%d x %d s' % (B, seconds), leg=leg, directions=D, mix_taps=La,
                           colour_taps=Lg, n_samples=n, ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3),
                           ms_max=round(float(t.max()), 3), rounds=len(t), calls_per_sample=args.calls if leg != 'torch call' else 1,
                           device=torch.cuda.get_device_name(0), **w)
                if leg == 'hip launch':
                    rec['launch_gfma_per_s'] = round(w['gfma'] / (np.median(t) * 1e-3), 1)
                emit(rec)
            if times['torch call']:
                emit(dict(bench='scene_diffuse', array='%s %s' % (fmt, baffle), size='%d x %d s' % (B, seconds),
                          hip_call_over_torch_call=round(float(np.median(times['hip call']) / np.median(times['torch call'])), 4)))
            del audio, out


if __name__ == '__main__':
    main()
