#!/usr/bin/env python
"""Time of the decay measurement and of a room calibration, and the decay that nominal rooms realise.  The legs
alternate in ONE process, one sample of each per round so that drift hits them alike, medians after warm-up, a host clock around WHOLE
calls of rir_acoustics (each ends in the download of the parameters, and of the curve when it is asked for: a device synchronise).
    a  HIP               salsa_rir_decay on the device, the responses already there
    b  torch, device     the composed torch evaluation on the device (SALSA_HIP_DECAY=0), the responses already there
    c  torch, host       the same on the CPU (device='cpu') from a host array, --host-rounds samples
Shapes: FOA banks of 72 and of 360 directions, 7200 taps, generated on the device in a 6 x 5 x 3.2 m room of nominal rt60 0.3 s, sources
at 1.5 m; each without and with the curve.  The time of salsa_rir_decay's launch alone (device events) is recorded with each shape, and
the largest difference of the legs' T20.  Then calibrate_room((6, 5, 3.2), 0.3) with its defaults, whole calls, on the device and on
the CPU; and the T20 on W that rooms of NOMINAL rt60 0.2 / 0.3 / 0.5 s realise in three directions, with the beta that calibrate_room
finds for the same figure.  One JSON line per record; whatever is seen is reported, a leg that loses included.

--bands measures per octave band instead: rir_acoustics(bands=OCTAVE_BANDS) on the FOA bank of 72 directions, HIP
(salsa_band_split, then salsa_rir_decay on seven band signals per response) against the torch path on the device, alternating; the
split's and the decay's launches alone; and calibrate_room against seven octave-band targets, 0.50 .. 0.20 s, 12000 taps.

    python tools/bench_room_acoustics.py [--bands] [--rounds 5] [--host-rounds 2] [--warmup 1] [--out profiles/room_acoustics_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
SIZE = (6.0, 5.0, 3.2)


def launch_ms(d_h, want_edc, warmup, rounds):
    """salsa_rir_decay alone: device events around one launch per sample -> ms per sample"""
    import ctypes as C
    import torch
    from salsa_amd import _lib
    L = _lib.load()
    R, Cn, Ln = d_h.shape
    out = torch.empty((R, Cn, L.salsa_rir_decay_params()), dtype=torch.float64, device=d_h.device)
    edc = torch.empty((R, Cn, Ln), dtype=torch.float64, device=d_h.device) if want_edc else None
    ms = []
    for r in range(warmup + rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rc = L.salsa_rir_decay(C.c_void_p(d_h.data_ptr()), R, Cn, Ln, 24000.0, 60, C.c_void_p(out.data_ptr()),
                               C.c_void_p(edc.data_ptr()) if want_edc else None, C.c_void_p(torch.cuda.current_stream(d_h.device).cuda_stream))
        b.record()
        torch.cuda.synchronize()
        if rc:
            raise RuntimeError(_lib.last_error())
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def banded(args, emit, stats):
    import ctypes as C
    import numpy as np
    import torch
    from salsa_amd import _lib, rooms
    dev, name = torch.device('cuda:0'), torch.cuda.get_device_name(0)
    bands, K, D = rooms.OCTAVE_BANDS, len(rooms.OCTAVE_BANDS), rooms.BAND_HALF
    directions = [(az, 0) for az in range(-180, 180, 5)]
    d_h, _ = rooms.room_rirs('foa', rooms.ShoeboxRoom(SIZE, rt60=(0.3,) * K, bands=bands), directions, 1.5, 7200, device=dev)
    legs = {'a HIP': True, 'b torch, device': False}
    times, last = {k: [] for k in legs}, {}
    for r in range(args.warmup + args.rounds):
        for leg, hip in legs.items():
            rooms.HIP_DECAY = hip
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = rooms.rir_acoustics(d_h, bands=bands)
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[leg].append((time.perf_counter() - t0) * 1e3)
            last[leg] = got.t20
    rooms.HIP_DECAY = True
    for leg in legs:
        emit(dict(bench='rir_acoustics_bands', responses=72, channels=4, bands=K, band_half=D, rir_len=7200, leg=leg, **stats(times[leg]),
                  max_rel_t20_difference_from_leg_a=float(np.nanmax(np.abs(last[leg] / last['a HIP'] - 1.0))), device=name))
    filters = torch.from_numpy(rooms.octave_filters(24000.0).astype(np.float32)).to(dev)
    x = d_h.reshape(72 * 4, 7200)
    split_ms = []
    for r in range(args.warmup + args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        y = rooms._band_split_hip(x, filters)
        b.record()
        torch.cuda.synchronize()
        if r >= args.warmup:
            split_ms.append(a.elapsed_time(b))
    decay_ms = launch_ms(y, False, args.warmup, args.rounds)
    emit(dict(bench='rir_acoustics_bands', responses=72, channels=4, bands=K, rir_len=7200, split_launch_alone=stats(split_ms),
              decay_launch_alone=stats(decay_ms), b_over_a=round(float(np.median(times['b torch, device']) / np.median(times['a HIP'])), 2), device=name))
    target = (0.50, 0.45, 0.40, 0.35, 0.30, 0.25, 0.20)
    cal_ms = []
    for r in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cal = rooms.calibrate_room(SIZE, rt60=target, bands=bands, length=12000, device=dev).calibration
        if r >= args.warmup:
            cal_ms.append((time.perf_counter() - t0) * 1e3)
    emit(dict(bench='calibrate_room_bands', room=list(SIZE), target=list(target), where='cuda', **stats(cal_ms), evaluations=cal['evaluations'],
              relative_error_per_evaluation=[[round(float(v), 5) for v in m / np.array(target) - 1.0] for m in cal['realised_history']],
              beta=[round(float(b), 6) for b in cal['beta_history'][-1][:, 0]], length=cal['length'], device=name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bands', action='store_true', help='per-band measurement and a seven-band calibration instead (DESIGN.md section 9p)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--host-rounds', type=int, default=2, help='samples of the host legs')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args()
    import numpy as np
    import torch
    from salsa_amd import rooms
    if not torch.cuda.is_available():
        raise SystemExit('bench_room_acoustics.py measures on cuda:0; there is none')
    dev = torch.device('cuda:0')
    name = torch.cuda.get_device_name(0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    med = lambda t: round(float(np.median(t)), 3)
    stats = lambda t: dict(ms_median=med(t), ms_min=round(float(min(t)), 3), ms_max=round(float(max(t)), 3), samples=len(t))
    if args.bands:
        return banded(args, emit, stats)
    room = rooms.ShoeboxRoom(SIZE, rt60=0.3)
    legs = {'a HIP': (True, dev), 'b torch, device': (False, dev), 'c torch, host': (False, 'cpu')}
    for n_dir in (72, 360):
        directions = [(az, 0) for az in range(-180, 180, 360 // n_dir)]
        d_h, _ = rooms.room_rirs('foa', room, directions, 1.5, 7200, device=dev)
        h_h = d_h.cpu().numpy()
        for want_edc in (False, True):
            times, last = {k: [] for k in legs}, {}
            for r in range(args.warmup + max(args.rounds, args.host_rounds)):
                for leg, (hip, where) in legs.items():
                    host = where == 'cpu'
                    if r >= (args.host_rounds if host else args.warmup + args.rounds):
                        continue
                    rooms.HIP_DECAY = hip
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got = rooms.rir_acoustics(h_h if host else d_h, edc=want_edc, device=where)
                    torch.cuda.synchronize()
                    if host or r >= args.warmup:
                        times[leg].append((time.perf_counter() - t0) * 1e3)
                    last[leg] = got.t20
            rooms.HIP_DECAY = True
            alone = launch_ms(d_h, want_edc, args.warmup, args.rounds)
            m = {leg: float(np.median(times[leg])) for leg in legs}
            for leg in legs:
                emit(dict(bench='rir_acoustics', responses=n_dir, channels=4, rir_len=7200, edc=want_edc, leg=leg, **stats(times[leg]),
                          max_rel_t20_difference_from_leg_a=float(np.nanmax(np.abs(last[leg] / last['a HIP'] - 1.0))), device=name))
            emit(dict(bench='rir_acoustics', responses=n_dir, channels=4, rir_len=7200, edc=want_edc, launch_alone=stats(alone),
                      bytes_read=int(d_h.numel() * 4), bytes_written=int(d_h.numel() * 8 if want_edc else 0) + n_dir * 4 * 15 * 8,
                      b_over_a=round(m['b torch, device'] / m['a HIP'], 2), c_over_a=round(m['c torch, host'] / m['a HIP'], 2), device=name))

    # a whole calibration, device against host
    times, cals = {'cuda': [], 'cpu': []}, {}
    for r in range(args.warmup + max(args.rounds, args.host_rounds)):
        for where in ('cuda', 'cpu'):
            if r >= (args.host_rounds if where == 'cpu' else args.warmup + args.rounds):
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cals[where] = rooms.calibrate_room(SIZE, 0.3, device=where).calibration
            if where == 'cpu' or r >= args.warmup:
                times[where].append((time.perf_counter() - t0) * 1e3)
    for where in ('cuda', 'cpu'):
        cal = cals[where]
        emit(dict(bench='calibrate_room', room=list(SIZE), target=0.3, where=where, **stats(times[where]), evaluations=cal['evaluations'],
                  beta=[round(float(b[0]), 6) for b in cal['beta_history']], realised=round(cal['realised'], 6),
                  probes=[round(float(v), 6) for v in cal['probes']], length=cal['length'], device=name))
    emit(dict(bench='calibrate_room', cpu_over_cuda=round(float(np.median(times['cpu'])) / float(np.median(times['cuda'])), 2)))

    # what nominal rooms realise, and what calibration makes of the same figure
    for nominal, length in ((0.2, 7200), (0.3, 7200), (0.5, 12000)):
        nom = rooms.ShoeboxRoom(SIZE, rt60=nominal)
        h, _ = rooms.room_rirs('foa', nom, [(0, 0), (90, 0), (180, 0)], 1.5, length, device=dev)
        got = rooms.rir_acoustics(h)
        cal = rooms.calibrate_room(SIZE, nominal, length=length, device=dev)
        emit(dict(bench='realised_decay', room=list(SIZE), nominal_rt60=nominal, taps=length, distance=1.5, eyring_beta=round(float(nom.beta[0]), 6),
                  t20_w=[round(float(v), 4) for v in got.t20[:, 0]], edt_w=[round(float(v), 4) for v in got.edt[:, 0]],
                  headroom_t20_db=[round(float(v), 1) for v in got.headroom_t20[:, 0]], truncated=[bool(v) for v in got.truncated('t20')[:, 0]],
                  calibrated_beta=[round(float(b[0]), 6) for b in cal.calibration['beta_history']], calibrated_t20=round(cal.calibration['realised'], 6),
                  calibrated_probes=[round(float(v), 6) for v in cal.calibration['probes']], evaluations=cal.calibration['evaluations'], device=name))


if __name__ == '__main__':
    main()
