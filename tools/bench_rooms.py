#!/usr/bin/env python
"""Time of the shoebox image-source generator.  Three legs in ONE process, one sample of each per round so that
drift hits them alike, medians after warm-up, a host clock around WHOLE calls of room_rir_bank (each ends in the download of the
responses, a device synchronise): the image table, the uploads, the sums, on a GPU the bank's partition spectra, and the download --
what a user's call costs.
    a  HIP               salsa_room_rirs on the device
    b  torch, device     the composed torch evaluation on the device (SALSA_HIP_ROOM=0)
    c  torch, host       the same on the CPU (device='cpu'), --host-rounds samples
Shapes: FOA and MIC banks of 72 directions (azimuth every 5 degrees) and one FOA bank of 360 (every degree), 7200 taps, sources at
1.5 m in a 6 x 5 x 3.2 m room with rt60 = 0.3 s (uniform beta by Eyring).  The largest difference between the legs' responses is
recorded with each shape, and so is the time of salsa_room_rirs' launch alone (device events, tables already uploaded; it includes the
launcher's host-side check of the table).  One JSON line per record; whatever is seen is reported, a leg that loses included.

--baffle rigid measures the MIC bank of 72 directions with the capsules on the rigid sphere instead: rigid(),
whose docstring lists its legs; the two launches alone share one image table (the rigid geometry's).  --bands measures the FOA bank of
72 directions in a room with seven octave bands: banded(), whose docstring lists its comparisons.

    python tools/bench_rooms.py [--baffle rigid | --bands] [--rounds 5] [--host-rounds 2] [--warmup 1] [--out profiles/room_rir_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def launch_ms(table, sources, receivers, foa, fs_over_c, length, dev, warmup, rounds):
    """salsa_room_rirs alone, its tables already on the device: device events around one launch per sample -> ms per sample"""
    import ctypes as C
    import torch
    from salsa_amd import _lib
    L = _lib.load()
    d_table, d_sources = torch.from_numpy(table).to(dev), torch.from_numpy(sources).to(dev)
    out = torch.empty((len(sources), 4 if foa else len(receivers), length), dtype=torch.float32, device=dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    ms = []
    for r in range(warmup + rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rc = L.salsa_room_rirs(hp(table), C.c_void_p(d_table.data_ptr()), table.shape[1], hp(sources), C.c_void_p(d_sources.data_ptr()),
                               len(sources), hp(receivers), len(receivers), int(foa), fs_over_c, length, C.c_void_p(out.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        b.record()
        torch.cuda.synchronize()
        if rc:
            raise RuntimeError(_lib.last_error())
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def sphere_launch_ms(table, sources, room, length, dev, samples):
    """salsa_room_rirs_sphere and salsa_room_rirs (open MIC) alone, ALTERNATING, their tables already on the device: device events
    around one launch per sample (each includes its launcher's host-side checks) -> (rigid ms, open ms) per sample"""
    import ctypes as C
    import numpy as np
    import torch
    from salsa_amd import _lib, rooms
    L = _lib.load()
    st = rooms.sphere_table(rooms.MIC_RADIUS, room.fs, room.c)
    centre, units, receivers = np.ascontiguousarray(room.array), np.ascontiguousarray(rooms._capsule_units()), room.receivers('mic')
    d_table, d_sources, d_sphere = torch.from_numpy(table).to(dev), torch.from_numpy(sources).to(dev), st.on(dev)
    out = torch.empty((len(sources), 4, length), dtype=torch.float32, device=dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    common = (hp(table), C.c_void_p(d_table.data_ptr()), table.shape[1], hp(sources), C.c_void_p(d_sources.data_ptr()), len(sources))
    calls = (lambda: L.salsa_room_rirs_sphere(*common, hp(centre), hp(units), hp(st.table), C.c_void_p(d_sphere.data_ptr()), st.Q, st.P, st.lead,
                                              st.trail, room.fs / room.c, length, C.c_void_p(out.data_ptr()), stream),
             lambda: L.salsa_room_rirs(*common, hp(receivers), 4, 0, room.fs / room.c, length, C.c_void_p(out.data_ptr()), stream))
    ms = ([], [])
    for r in range(samples[0] + samples[1]):
        for which, call in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            rc = call()
            b.record()
            torch.cuda.synchronize()
            if rc:
                raise RuntimeError(_lib.last_error())
            if r >= samples[0]:
                ms[which].append(a.elapsed_time(b))
    return ms


def rigid(args):
    """--baffle rigid: the MIC bank of 72 directions with the capsules on the rigid sphere.  Legs, one sample of
    each per round: a HIP rigid, a' HIP open (the same bank in free space, alternating with a), b the rigid torch path on the device,
    c the same on the host.  Whole calls of room_rir_bank, and the two launches alone, alternating."""
    import numpy as np
    import torch
    from salsa_amd import rooms
    dev = torch.device('cuda:0')
    room = rooms.ShoeboxRoom((6.0, 5.0, 3.2), rt60=0.3)
    n_dir = 72
    directions = [(az, 0) for az in range(-180, 180, 360 // n_dir)]
    _, sources, _, d_max = rooms.room_geometry('mic', room, directions, args.distance, args.rir_len, baffle='rigid')
    images = rooms.room_images(room, d_max)
    st = rooms.sphere_table(rooms.MIC_RADIUS, room.fs, room.c)
    legs = {'a HIP rigid': (True, dev, 'rigid'), "a' HIP open": (True, dev, 'open'), 'b torch rigid, device': (False, dev, 'rigid'),
            'c torch rigid, host': (False, 'cpu', 'rigid')}
    times, last = {k: [] for k in legs}, {}
    for r in range(args.warmup + max(args.rounds, args.host_rounds)):
        for leg, (hip, where, baffle) in legs.items():
            host = where == 'cpu'
            if r >= (args.host_rounds if host else args.warmup + args.rounds):
                continue
            rooms.HIP_ROOM = hip
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank = rooms.room_rir_bank('mic', room, directions, args.distance, args.rir_len, device=where, baffle=baffle)
            torch.cuda.synchronize()
            if host or r >= args.warmup:
                times[leg].append((time.perf_counter() - t0) * 1e3)
            last[leg] = bank.rirs
    rooms.HIP_ROOM = True
    rigid_ms, open_ms = sphere_launch_ms(images.table(), sources, room, args.rir_len, dev, (args.warmup, args.rounds))
    recs = []
    for leg, (_, _, baffle) in legs.items():
        t = np.array(times[leg])
        recs.append(dict(bench='room_rir_sphere', format='mic', baffle=baffle, directions=n_dir, rir_len=args.rir_len, room=[6.0, 5.0, 3.2],
                         rt60_nominal=0.3, beta=round(float(room.beta[0]), 6), distance=args.distance, images=len(images), leg=leg,
                         ms_median=round(float(np.median(t)), 2), ms_min=round(float(t.min()), 2), ms_max=round(float(t.max()), 2), samples=len(t),
                         max_abs_difference_from_leg_a=None if baffle == 'open' else float(np.abs(last[leg] - last['a HIP rigid']).max()),
                         max_abs_response=round(float(np.abs(last[leg]).max()), 4), device=torch.cuda.get_device_name(0)))
    med = {leg: float(np.median(times[leg])) for leg in legs}
    rm, om = float(np.median(rigid_ms)), float(np.median(open_ms))
    recs.append(dict(bench='room_rir_sphere', format='mic', directions=n_dir, rir_len=args.rir_len, table=list(st.table.shape), lead=st.lead, trail=st.trail,
                     rigid_launch_alone_ms_median=round(rm, 3), rigid_launch_alone_ms_min=round(min(rigid_ms), 3), rigid_launch_alone_ms_max=round(max(rigid_ms), 3),
                     open_launch_alone_ms_median=round(om, 3), open_launch_alone_ms_min=round(min(open_ms), 3), open_launch_alone_ms_max=round(max(open_ms), 3),
                     launch_alone_samples=len(rigid_ms), rigid_over_open_launch=round(rm / om, 2),
                     taps_visited_per_image_rigid_over_open=round((st.lead + st.trail) / 32.0, 2),
                     rigid_over_open_whole_call=round(med['a HIP rigid'] / med["a' HIP open"], 2),
                     b_over_a=round(med['b torch rigid, device'] / med['a HIP rigid'], 2), c_over_a=round(med['c torch rigid, host'] / med['a HIP rigid'], 2)))
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


def _event_ms(calls, samples):
    """device events around each call, the calls ALTERNATING, one sample of each per round -> one list of ms per call"""
    import torch
    ms = [[] for _ in calls]
    for r in range(samples[0] + samples[1]):
        for which, call in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            if r >= samples[0]:
                ms[which].append(a.elapsed_time(b))
    return ms


def banded(args):
    """--bands: the FOA bank of 72 directions in a room with seven octave bands, every band at rt60 = 0.3 s so that
    the table is the one of the broadband records.  Three comparisons, each with its legs alternating in one process:
      launches   salsa_room_rirs_bands (K = 7, the taps -D .. L + D - 1) against seven launches of salsa_room_rirs over as many taps, one
                 per band -- what the parent commit offers for the same rows (its taps start at 0; the work is the same);
      filters    salsa_band_merge and salsa_band_split against torch's conv1d on the device, on the bank's own shapes;
      whole      room_rir_bank of the banded room: HIP, the composed torch path on the device, and the broadband room's HIP call."""
    import ctypes as C
    import numpy as np
    import torch
    from salsa_amd import _lib, rooms
    L = _lib.load()
    dev = torch.device('cuda:0')
    K, D, length, n_dir = len(rooms.OCTAVE_BANDS), rooms.BAND_HALF, args.rir_len, 72
    room = rooms.ShoeboxRoom((6.0, 5.0, 3.2), rt60=(0.3,) * K, bands=rooms.OCTAVE_BANDS)
    plain = rooms.ShoeboxRoom((6.0, 5.0, 3.2), rt60=0.3)
    directions = [(az, 0) for az in range(-180, 180, 360 // n_dir)]
    _, sources, receivers, d_max = rooms.room_geometry('foa', room, directions, args.distance, length)
    images = rooms.room_images(room, d_max)
    table, n_taps, fs_over_c = images.band_table(), length + 2 * D, room.fs / room.c
    single = np.ascontiguousarray(table[:7])
    d_table, d_single, d_sources = (torch.from_numpy(a).to(dev) for a in (table, single, sources))
    r = torch.empty((n_dir, 4, K, n_taps), dtype=torch.float32, device=dev)
    one = torch.empty((n_dir, 4, n_taps), dtype=torch.float32, device=dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def ok(rc):
        if rc:
            raise RuntimeError(_lib.last_error())

    def launch_banded():
        ok(L.salsa_room_rirs_bands(hp(table), dp(d_table), table.shape[1], K, hp(sources), dp(d_sources), n_dir, hp(receivers), 1, 1, fs_over_c, -D,
                                   n_taps, dp(r), stream))

    def launch_k_single():
        for _ in range(K):
            ok(L.salsa_room_rirs(hp(single), dp(d_single), single.shape[1], hp(sources), dp(d_sources), n_dir, hp(receivers), 1, 1, fs_over_c, n_taps,
                                 dp(one), stream))
    banded_ms, single_ms = _event_ms((launch_banded, launch_k_single), (args.warmup, args.rounds))
    # the filters, on the rows the launch left
    filters = torch.from_numpy(rooms.octave_filters(room.fs).astype(np.float32)).to(dev)
    rows = r.reshape(n_dir * 4, K, n_taps)
    merged = rooms._band_merge_hip(rows, filters)
    merge_diff = float((merged - rooms._band_merge_torch(rows, filters)).abs().max())
    split_diff = float((rooms._band_split_hip(merged, filters) - rooms._band_split_torch(merged, filters)).abs().max())
    filter_ms = _event_ms((lambda: rooms._band_merge_hip(rows, filters), lambda: rooms._band_merge_torch(rows, filters),
                           lambda: rooms._band_split_hip(merged, filters), lambda: rooms._band_split_torch(merged, filters)), (args.warmup, args.rounds))
    # whole calls
    legs = {'a HIP banded': (True, room), 'b torch banded, device': (False, room), "a' HIP broadband": (True, plain)}
    times, last = {k: [] for k in legs}, {}
    for rnd in range(args.warmup + args.rounds):
        for leg, (hip, which) in legs.items():
            if not hip and rnd >= args.warmup + args.host_rounds:
                continue
            rooms.HIP_ROOM = hip
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bank = rooms.room_rir_bank('foa', which, directions, args.distance, length, device=dev)
            torch.cuda.synchronize()
            if rnd >= args.warmup:
                times[leg].append((time.perf_counter() - t0) * 1e3)
            last[leg] = bank.rirs
    rooms.HIP_ROOM = True
    med = lambda v: round(float(np.median(v)), 3)
    span = lambda v: [round(float(min(v)), 3), round(float(max(v)), 3)]
    common = dict(bench='room_rir_bands', format='foa', directions=n_dir, rir_len=length, bands=K, band_half=D, room=[6.0, 5.0, 3.2], rt60_nominal=0.3,
                  distance=args.distance, images=len(images), device=torch.cuda.get_device_name(0))
    recs = [dict(common, what='launches alone', taps=n_taps, banded_launch_ms_median=med(banded_ms), banded_launch_ms_min_max=span(banded_ms),
                 k_single_launches_ms_median=med(single_ms), k_single_launches_ms_min_max=span(single_ms), samples=len(banded_ms),
                 banded_over_k_single=round(float(np.median(banded_ms) / np.median(single_ms)), 3)),
            dict(common, what='filters', rows=n_dir * 4, merge_hip_ms_median=med(filter_ms[0]), merge_hip_ms_min_max=span(filter_ms[0]),
                 merge_conv1d_ms_median=med(filter_ms[1]), merge_conv1d_ms_min_max=span(filter_ms[1]), split_hip_ms_median=med(filter_ms[2]),
                 split_hip_ms_min_max=span(filter_ms[2]), split_conv1d_ms_median=med(filter_ms[3]), split_conv1d_ms_min_max=span(filter_ms[3]),
                 samples=len(filter_ms[0]), merge_hip_over_conv1d=round(float(np.median(filter_ms[0]) / np.median(filter_ms[1])), 3),
                 split_hip_over_conv1d=round(float(np.median(filter_ms[2]) / np.median(filter_ms[3])), 3),
                 merge_max_abs_difference=merge_diff, split_max_abs_difference=split_diff)]
    for leg in legs:
        recs.append(dict(common, what='whole call', leg=leg, ms_median=med(times[leg]), ms_min_max=span(times[leg]), samples=len(times[leg]),
                         max_abs_difference_from_leg_a=float(np.abs(last[leg] - last['a HIP banded']).max()),
                         max_abs_response=round(float(np.abs(last[leg]).max()), 4)))
    for rec in recs:
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bands', action='store_true', help='the legs of the octave-band room instead (DESIGN.md section 9p)')
    ap.add_argument('--baffle', choices=['open', 'rigid'], default='open', help='rigid: the legs of the rigid-sphere MIC bank instead')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=2, help='samples of leg c')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--rir-len', type=int, default=7200)
    ap.add_argument('--distance', type=float, default=1.5)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import rooms
    if not torch.cuda.is_available():
        raise SystemExit('bench_rooms.py measures on cuda:0; there is none')
    if args.bands:
        return banded(args)
    if args.baffle == 'rigid':
        return rigid(args)
    dev = torch.device('cuda:0')
    room = rooms.ShoeboxRoom((6.0, 5.0, 3.2), rt60=0.3)
    shapes = [('foa', 72), ('mic', 72), ('foa', 360)]
    legs = {'a HIP': (True, dev), 'b torch, device': (False, dev), 'c torch, host': (False, 'cpu')}
    for fmt, n_dir in shapes:
        recs = []
        directions = [(az, 0) for az in range(-180, 180, 360 // n_dir)]
        _, sources, receivers, d_max = rooms.room_geometry(fmt, room, directions, args.distance, args.rir_len)
        table_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            images = rooms.room_images(room, d_max)
            table_ms.append((time.perf_counter() - t0) * 1e3)
        n_images, table_ms = len(images), min(table_ms)
        times, last = {k: [] for k in legs}, {}
        for r in range(args.warmup + max(args.rounds, args.host_rounds)):
            for leg, (hip, where) in legs.items():
                host = where == 'cpu'
                if r >= (args.host_rounds if host else args.warmup + args.rounds):
                    continue
                rooms.HIP_ROOM = hip
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bank = rooms.room_rir_bank(fmt, room, directions, args.distance, args.rir_len, device=where)
                torch.cuda.synchronize()
                if host or r >= args.warmup:
                    times[leg].append((time.perf_counter() - t0) * 1e3)
                last[leg] = bank.rirs
        rooms.HIP_ROOM = True
        kernel_ms = launch_ms(images.table(), sources, receivers, fmt == 'foa', room.fs / room.c, args.rir_len, dev, args.warmup, args.rounds)
        top = float(np.abs(last['a HIP']).max())
        for leg in legs:
            t = np.array(times[leg])
            recs.append(dict(bench='room_rir', format=fmt, directions=n_dir, rir_len=args.rir_len, room=[6.0, 5.0, 3.2], rt60_nominal=0.3,
                             beta=round(float(room.beta[0]), 6), distance=args.distance, images=n_images, leg=leg,
                             ms_median=round(float(np.median(t)), 2), ms_min=round(float(t.min()), 2), ms_max=round(float(t.max()), 2),
                             samples=len(t), host_ms_to_build_the_image_table=round(table_ms, 2),
                             max_abs_difference_from_leg_a=float(np.abs(last[leg] - last['a HIP']).max()), max_abs_response=round(top, 4),
                             device=torch.cuda.get_device_name(0)))
        med = {leg: float(np.median(times[leg])) for leg in legs}
        recs.append(dict(bench='room_rir', format=fmt, directions=n_dir, rir_len=args.rir_len,
                         launch_alone_ms_median=round(float(np.median(kernel_ms)), 3), launch_alone_ms_min=round(min(kernel_ms), 3),
                         launch_alone_ms_max=round(max(kernel_ms), 3), launch_alone_samples=len(kernel_ms),
                         b_over_a=round(med['b torch, device'] / med['a HIP'], 2), c_over_a=round(med['c torch, host'] / med['a HIP'], 2)))
        for rec in recs:
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()
