#!/usr/bin/env python
"""Time of the scene renderer with moving sources.  Four legs in ONE process, one sample of each per round so
that drift hits them alike, medians after warm-up, device events around each sample between two synchronises:
    a  static, old entry     the drawn scenes through salsa_scene_render: the path as it was, and the yardstick
    b  static, new entry     the same scenes through salsa_scene_render_moving (one segment of step 0 per item); equal bits are checked
    c  moving                the same items, every one with a trajectory at --step samples (azimuth speeds of 10 - 40 degrees per second,
                             seeded), through salsa_scene_render_moving; segment count and workspace bytes are recorded
    d  moving, torch.fft     (c) composed from torch.fft calls, one per segment (SALSA_HIP_SCENE=0); --slow-rounds samples of one call
at two sizes: --batch clips of 60 s and --batch clips of 8 s, responses of 7200 taps, as tools/bench_scenes.py.  A call includes its
table building, uploads and allocations: it is what a user's call costs.  The overlap-save work is counted by tools/bench_scenes.py's
work() on the segments.  One JSON line per record; whatever is seen is reported, slower included.

    python tools/bench_scenes_moving.py [--rounds 7] [--calls 3] [--warmup 2] [--batch 32] [--out profiles/scene_moving_bench.jsonl]"""
import argparse
import json
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)


def with_trajectories(scenes, pool, bank, step, seed, speed_deg_s=(10.0, 40.0)):
    """the same items (events, onsets, gains, tracks), each moving in azimuth from its response at a seeded speed"""
    import numpy as np
    from salsa_amd import scenes as sc
    rng = np.random.default_rng(seed)
    clips = []
    for b in range(scenes.n_clips):
        items = []
        for i in range(scenes.clip_start[b], scenes.clip_start[b + 1]):
            r = int(scenes.rir[i])
            speed = rng.uniform(*speed_deg_s) * (1.0 if rng.random() < 0.5 else -1.0)
            az = bank.azimuth[r] + speed * np.arange(int(sc.traj_nodes(scenes.length[i], step))) * step / sc.FS
            traj = list(bank.nearest((az + 180.0) % 360.0 - 180.0, np.full(len(az), float(bank.elevation[r]))))
            items.append((int(scenes.event[i]), traj, int(scenes.onset[i]), float(scenes.gain[i]), int(scenes.track[i])))
        clips.append(items)
    return sc.Scenes.from_items(scenes.n_samples, clips, pool, bank, traj_step=step)


def segment_work(scenes, pool, bank):
    """bench_scenes.work() on the segments: each is an item of its own to the overlap-save"""
    import numpy as np
    import bench_scenes
    from salsa_amd import scenes as sc
    clip_start, segs, gains, block, longest = sc.segment_tables(scenes, pool, bank)
    n = segs.shape[1]
    as_items = types.SimpleNamespace(n_samples=scenes.n_samples, event=np.arange(n), onset=segs[1], clip_start=clip_start,
                                     n_clips=scenes.n_clips, n_items=n)
    w = bench_scenes.work(as_items, types.SimpleNamespace(lengths=segs[2]), bank)
    w['segments'] = w.pop('items')
    w['items'] = int(scenes.n_items)
    w['longest_segment'] = longest
    t0 = time.perf_counter()
    for _ in range(5):
        sc.segment_tables(scenes, pool, bank)
    w['host_ms_to_build_the_tables'] = round((time.perf_counter() - t0) / 5 * 1e3, 3)      # part of every call of legs b and c
    w['segments_visited_per_rendered_block'] = round(float(np.diff(block, axis=-1).sum()) / max(1, w['output_blocks_rendered']), 2)
    return w, n, longest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--slow-rounds', type=int, default=2, help='samples of leg d (one call each)')
    ap.add_argument('--calls', type=int, default=3, help='back-to-back calls per timed sample of legs a, b, c')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rir-len', type=int, default=7200)
    ap.add_argument('--step', type=int, default=2400)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import _lib
    from salsa_amd import scenes as sc
    dev = torch.device('cuda:0')
    pool = sc.synth_event_pool(12, 4, 0, min_s=1.0, max_s=3.0)
    bank = sc.make_rir_bank('foa', [(a, e) for a in range(-180, 180, 30) for e in (-30, 0, 30)], args.rir_len, rt60=0.3, seed=1)
    bank.spectra(dev)                                                          # once per bank: not part of a render
    recs = []
    for tag, seconds in (('60 s', 60), ('8 s', 8)):
        n = seconds * sc.FS
        static = sc.draw_scenes(args.batch, pool, bank, n, 2021)
        moving = with_trajectories(static, pool, bank, args.step, 2021)
        amb = 1e-3 * torch.randn(args.batch, 4, n, device=dev)
        out = torch.empty_like(amb)
        legs = {'a static, old entry': (static, True, {}), 'b static, new entry': (static, True, dict(segments=True)),
                'c moving': (moving, True, {}), 'd moving, torch.fft': (moving, False, {})}
        times, host, peak = {k: [] for k in legs}, {k: [] for k in legs}, {}
        for r in range(args.warmup + args.rounds):
            for leg, (scenes, hip, kw) in legs.items():
                slow = not hip
                if slow and r >= args.slow_rounds:
                    continue
                calls = 1 if slow else args.calls
                sc.HIP_SCENE = hip
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                a.record()
                for _ in range(calls):
                    sc.render_scenes(scenes, pool, bank, ambient=amb, out=out, **kw)
                b.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                peak[leg] = torch.cuda.max_memory_allocated() - base
                if slow or r >= args.warmup:
                    times[leg].append(a.elapsed_time(b) / calls)
                    host[leg].append((t1 - t0) * 1e3 / calls)
        sc.HIP_SCENE = True
        old = sc.render_scenes(static, pool, bank, ambient=amb).clone()
        new = sc.render_scenes(static, pool, bank, ambient=amb, segments=True)
        equal_bits = bool(torch.equal(old.view(torch.int32), new.view(torch.int32)))
        del old, new
        hip_moving = sc.render_scenes(moving, pool, bank, ambient=amb).clone()
        sc.HIP_SCENE = False
        other = sc.render_scenes(moving, pool, bank, ambient=amb)
        sc.HIP_SCENE = True
        diff, top = float((hip_moving - other).abs().max()), float(other.abs().max())
        del other, hip_moving
        L = _lib.load()
        w_static, n_static, long_static = segment_work(static, pool, bank)
        w_moving, n_moving, long_moving = segment_work(moving, pool, bank)
        size = '%d x %s' % (args.batch, tag)
        for leg, (scenes, hip, kw) in legs.items():
            t = np.array(times[leg])
            w = w_static if scenes is static else w_moving
            rec = dict(bench='scene_moving', size=size, leg=leg, rir_len=args.rir_len, n_samples=n, traj_step=args.step,
                       ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
                       host_ms_median=round(float(np.median(host[leg])), 3), samples=len(t), calls_per_sample=args.calls if hip else 1,
                       temporaries_mb=round(peak[leg] / 2 ** 20, 1), device=torch.cuda.get_device_name(0), **w)
            if leg.startswith('a'):
                del rec['host_ms_to_build_the_tables']                         # the old entry takes the item tables as they are
                rec['workspace_bytes'] = int(L.salsa_scene_workspace_bytes(n, pool.max_len, static.n_items))
            elif hip:
                ns, longest = (n_static, long_static) if scenes is static else (n_moving, long_moving)
                rec['workspace_bytes'] = int(L.salsa_scene_moving_workspace_bytes(n, longest, ns))
            recs.append(rec)
        med = {leg: float(np.median(times[leg])) for leg in legs}
        a_ms, b_ms, c_ms, d_ms = (med[k] for k in legs)
        recs.append(dict(bench='scene_moving', size=size, new_entry_equals_old_entry_bit_for_bit=equal_bits,
                         b_over_a=round(b_ms / a_ms, 3), c_over_a=round(c_ms / a_ms, 3), c_over_d=round(c_ms / d_ms, 4),
                         spectrum_pairs_c_over_a=round(w_moving['spectrum_pairs'] / max(1, w_static['spectrum_pairs']), 3),
                         ols_gflop_c_over_a=round(w_moving['ols_gflop'] / max(1e-9, w_static['ols_gflop']), 3),
                         max_abs_difference_of_c_and_d=diff, max_abs_output=round(top, 4)))
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
