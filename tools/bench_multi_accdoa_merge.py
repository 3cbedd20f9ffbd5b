#!/usr/bin/env python
"""Times of the two merges of track_merge='align'  on --batch clips x --frames label frames x --classes real
classes of random Multi-ACCDOA outputs, the HIP launch against the composed torch operators ON THE DEVICE, all legs in ONE process
and alternating (every round times each leg once, after a warm-up of all of them, so drift of a shared host hits the legs alike);
each call is timed by a host clock around the call and a device synchronise:

    tta16_merge_hip     one salsa_nn_tta_merge_multi launch on the 16 FOA slabs (un-swap, align to slab 0, sum, divide, lengths)
    tta16_merge_torch   tta.tta_merge_multi under SALSA_HIP_TTA=0: the same statements as torch operators
    chunk_merge_hip     one salsa_nn_chunk_merge_multi launch on --chunk-len / --chunk-hop label-frame chunks (40 / 20 = 4 s / 2 s)
    chunk_merge_torch   the same walk chunk by chunk with torch operators (the device restatement of postprocess.combine_chunks_multi)

Before anything is timed the legs of a pair are held to each other bit for bit.  One JSON line per leg: median / 10th / 90th
percentile / min / max in ms.

    python tools/bench_multi_accdoa_merge.py [--steps 20] [--warmup 3] [--out profiles/multi_accdoa_merge_bench.jsonl]"""
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


def chunk_merge_torch(act, xyz, chunk_len, hop, n_frames, C):
    """postprocess.combine_chunks_multi for a batch of files with torch operators on the tensors' device: act (files, n_chunks,
    chunk_len, 3 C), xyz (.., 9 C) -> (files, n_frames, 3 C), (files, n_frames, 9 C)"""
    import torch
    from salsa_amd.crnn.decode import chunk_starts
    from salsa_amd.crnn.postprocess import TRACK_PERMS
    from salsa_amd.crnn.tta import _align_torch
    files, n = act.shape[:2]
    starts = chunk_starts(n_frames, chunk_len, hop)
    assert len(starts) == n and n > 1
    table = torch.tensor(TRACK_PERMS, dtype=torch.long, device=act.device)
    a = act.reshape(files, n, chunk_len, 3, C)                                       # (file, chunk, frame, track, C)
    v = xyz.reshape(files, n, chunk_len, 3, 3, C)                                    # (file, chunk, frame, axis, track, C)
    out_a = torch.empty((files, n_frames, 3, C), dtype=torch.float32, device=act.device)
    out_v = torch.empty((files, n_frames, 3, 3, C), dtype=torch.float32, device=act.device)
    overlap = chunk_len - hop
    for i, s in enumerate(starts):
        if i == 0:
            out_a[:, s:s + chunk_len], out_v[:, s:s + chunk_len] = a[:, i], v[:, i]
            continue
        if overlap > 0:
            old_v, new_v = out_v[:, s:s + overlap], v[:, i, :overlap]
            src = table[_align_torch(old_v, new_v)].permute(0, 1, 3, 2)               # (file, frame, track, C): the source of track n
            out_v[:, s:s + overlap] = (old_v + torch.gather(new_v, 3, src[:, :, None].expand_as(new_v))) / 2.0
            out_a[:, s:s + overlap] = (out_a[:, s:s + overlap] + torch.gather(a[:, i, :overlap], 2, src)) / 2.0
        out_a[:, s + overlap:s + chunk_len], out_v[:, s + overlap:s + chunk_len] = a[:, i, overlap:], v[:, i, overlap:]
    return out_a.reshape(files, n_frames, 3 * C), out_v.reshape(files, n_frames, 9 * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed rounds (every leg once per round)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--frames', type=int, default=600, help='label frames per clip (600 = 60 s)')
    ap.add_argument('--classes', type=int, default=12)
    ap.add_argument('--chunk-len', type=int, default=40, help='label frames per test chunk (40 = 4 s)')
    ap.add_argument('--chunk-hop', type=int, default=20)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import torch
    from salsa_amd.crnn import tta
    from salsa_amd.crnn.decode import chunk_merge_multi, chunk_starts
    if not torch.cuda.is_available():
        raise SystemExit('bench_multi_accdoa_merge needs a GPU')
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(5)
    B, L, C = args.batch, args.frames, args.classes
    ids = list(range(16))
    slab = torch.tanh(torch.randn((16, B, L, 9 * C), device=dev, generator=g))
    n_chunks = len(chunk_starts(L, args.chunk_len, args.chunk_hop))
    cx = torch.tanh(torch.randn((B, n_chunks, args.chunk_len, 9 * C), device=dev, generator=g))
    ca = torch.rand((B, n_chunks, args.chunk_len, 3 * C), device=dev, generator=g)

    def with_switch(on, f):
        def call():
            tta.USE_HIP_TTA = on
            try:
                return f()
            finally:
                tta.USE_HIP_TTA = True
        return call

    legs = {'tta16_merge_hip': with_switch(True, lambda: tta.tta_merge_multi(slab, 1, ids, 'foa', C)),
            'tta16_merge_torch': with_switch(False, lambda: tta.tta_merge_multi(slab, 1, ids, 'foa', C)),
            'chunk_merge_hip': lambda: chunk_merge_multi(ca, cx, args.chunk_len, args.chunk_hop, n_frames=L, n_classes=C),
            'chunk_merge_torch': lambda: chunk_merge_torch(ca, cx, args.chunk_len, args.chunk_hop, L, C)}
    for pair in ('tta16_merge', 'chunk_merge'):                                      # the legs compute the same bits
        hip, composed = legs[pair + '_hip'](), legs[pair + '_torch']()
        for x, y in zip(hip, composed):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), pair
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
    lines = []
    for name, t in times.items():
        rec = dict(bench='multi_accdoa_merge', leg=name, batch=B, label_frames=L, classes=C, calls=len(t), **_stats(t))
        if name.startswith('tta16'):
            rec.update(slabs=16, slab_mbytes=round(slab.numel() * 4 / 2 ** 20, 1))
        else:
            rec.update(chunk_len=args.chunk_len, chunk_hop=args.chunk_hop, n_chunks=n_chunks)
        if name.endswith('_hip'):
            rec['torch_over_hip'] = round(_stats(times[name[:-4] + '_torch'])['ms_median'] / max(rec['ms_median'], 1e-6), 2)
        rec['gpu'] = torch.cuda.get_device_name(0)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
