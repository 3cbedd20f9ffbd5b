#!/usr/bin/env python
"""Does the training step learn to localise?  A record, not a test: FOA training scenes and held-out scenes are
drawn from different seeds over ONE event pool and ONE response bank (salsa_amd/scenes.py), rendered on the device, extracted into
GpuFeatureBanks, and Trainer.fit runs a few epochs.  The SELD 2021 scores on the held-out scenes are recorded before training and
after every epoch.  No score is promised; the JSON lines say what was seen.

    python tools/train_on_scenes.py [--train-clips 48] [--val-clips 8] [--epochs 8] [--moving 0.5] [--room] [--format mic --baffle rigid] [--ambient diffuse --snr-db 20] [--conformer 2] [--out profiles/scene_training.jsonl]

--moving FRACTION makes that share of the items move in azimuth in the training and the held-out scenes alike, so
the ground truth's directions change inside events; 0 (the default) leaves the run as it was.
--room takes the responses from room_rir_bank instead of make_rir_bank: the same 48 directions, sources at
--distance metres from the centre of a 6 x 5 x 3.2 m shoebox whose uniform reflection coefficient is Eyring's for --rt60 (a nominal
figure: the realised decay is longer), generated on the device.
--format mic renders the four capsules of the TNSSE tetrahedron and extracts SALSA-MIC (fmax_doa 4 kHz); --baffle rigid puts them on the
rigid sphere, --baffle open (the default) leaves them in free space.
--ambient white (the default) renders the scenes over channel-independent white noise of rms 1e-3, the draw this tool has always made;
--ambient diffuse adds the spatially diffuse field of DESIGN.md section 9q instead (64 directions, 'room' colour, the array of --format and
--baffle) at --snr-db decibels below each clip's own mean square.  Each run is ONE run."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--train-clips', type=int, default=48)
    ap.add_argument('--val-clips', type=int, default=8)
    ap.add_argument('--clip-s', type=int, default=60)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rir-len', type=int, default=2400)
    ap.add_argument('--rt60', type=float, default=0.3)
    ap.add_argument('--seed', type=int, default=2021)
    ap.add_argument('--moving', type=float, default=0.0, help='fraction of items that move (DESIGN.md section 9l); 0: the run as it was')
    ap.add_argument('--room', action='store_true', help='image-source responses of a shoebox room (DESIGN.md section 9m) instead of make_rir_bank')
    ap.add_argument('--distance', type=float, default=1.5, help='--room: metres from the array centre to every source')
    ap.add_argument('--format', choices=['foa', 'mic'], default='foa', help='mic: the TNSSE tetrahedron, SALSA-MIC features up to 4 kHz')
    ap.add_argument('--baffle', choices=['open', 'rigid'], default='open',
                    help='--format mic: the capsules in free space, or on the rigid sphere of DESIGN.md section 9o')
    ap.add_argument('--ambient', choices=['white', 'diffuse'], default='white',
                    help='white: independent noise of rms 1e-3 per channel; diffuse: the diffuse field of DESIGN.md section 9q at --snr-db')
    ap.add_argument('--snr-db', type=float, default=20.0, help='--ambient diffuse: each clip\'s mean square over the noise\'s expected one, dB')
    ap.add_argument('--conformer', type=int, default=0, help='Conformer blocks after the recurrent decoder (DESIGN.md section 9r); 0: the run as it was')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    args = ap.parse_args(argv)
    if args.baffle == 'rigid' and args.format != 'mic':
        ap.error('--baffle rigid needs --format mic')
    return args


def scene_ambient(args, field, n_clips, n, device, generator, first_seed):
    """-> (ambient, diffuse) for add_scenes: --ambient white draws the ambient tensor from `generator` and adds no field; --ambient diffuse
    renders over silence and hands `field` on, clip i seeded first_seed + i"""
    import torch
    if args.ambient == 'white':
        return 1e-3 * torch.randn(n_clips, 4, n, device=device, generator=generator), None
    return None, (field, dict(snr_db=args.snr_db, seed=first_seed))


def main():
    args = parse_args()
    baffle = dict(baffle=args.baffle) if args.format == 'mic' else {}
    import numpy as np
    import torch
    from salsa_amd import scenes as sc
    from salsa_amd.crnn.fit import validate
    from salsa_amd.crnn.train import Trainer
    from salsa_amd.dataset import GpuFeatureBank
    from salsa_amd.extractor import SalsaExtractor

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    def static_view(scene):
        """the same items without their trajectories: every row carries node 0's direction"""
        return sc.Scenes(scene.n_samples, scene.clip_start, **{f: getattr(scene, f) for f in sc.Scenes.FIELDS})

    dev = torch.device('cuda:0')
    NC, n = 12, args.clip_s * sc.FS
    pool = sc.synth_event_pool(NC, 4, 0)
    directions = [(a, e) for a in range(-180, 180, 30) for e in (-40, -10, 20, 50)]
    room_rec = {}
    if args.room:
        room = sc.ShoeboxRoom((6.0, 5.0, 3.2), rt60=args.rt60)
        t0 = time.perf_counter()
        rbank = sc.room_rir_bank(args.format, room, directions, args.distance, args.rir_len, device=dev, **baffle)
        room_rec = dict(room=[6.0, 5.0, 3.2], beta=round(float(room.beta[0]), 6), rt60_is='nominal (Eyring); the realised decay is longer',
                        distance=args.distance, seconds_to_generate_the_bank=round(time.perf_counter() - t0, 3),
                        response_energy_after_the_first_50_taps=round(float((rbank.rirs[:, 0, 50:] ** 2).sum() / (rbank.rirs[:, 0] ** 2).sum()), 4))
    else:
        rbank = sc.make_rir_bank(args.format, directions, args.rir_len, rt60=args.rt60, seed=1, **baffle)
    ex = SalsaExtractor(audio_format=args.format, fmax_doa=9000 if args.format == 'foa' else 4000, device=dev)
    field = sc.DiffuseField(args.format, **baffle) if args.ambient == 'diffuse' else None
    noise_rec = dict(ambient_rms=1e-3) if field is None else dict(ambient='diffuse', snr_db=args.snr_db, diffuse_directions=field.n_directions,
                                                                  diffuse_colour='room')
    t0 = time.perf_counter()
    banks, drawn = {}, {}
    for name, clips, seed in (('train', args.train_clips, args.seed), ('val', args.val_clips, args.seed + 1000)):
        scenes = sc.draw_scenes(clips, pool, rbank, n, seed, **(dict(moving=args.moving) if args.moving else {}))
        bank = GpuFeatureBank(ex, n_classes=NC, max_clip_s=args.clip_s)
        g = torch.Generator(dev).manual_seed(seed)
        for lo in range(0, clips, 16):                                         # 16 clips of audio at a time
            part = scenes.clips(lo, min(lo + 16, clips))
            amb, diffuse = scene_ambient(args, field, part.n_clips, n, dev, g, seed * 65536 + lo)
            sc.add_scenes(bank, part, pool, rbank, names=['%s_%04d' % (name, lo + i) for i in range(part.n_clips)], ambient=amb, diffuse=diffuse)
        banks[name], drawn[name] = bank, scenes
    banks['train'].fit_scaler()
    mean, std = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (banks['train'].mean, banks['train'].std))
    banks['val'].set_scaler(mean, std)
    for b in banks.values():
        b.finalize()
    torch.cuda.synchronize()
    val_gt = [[(int(f), int(c), float(az), float(el), int(t)) for f, c, t, az, el in sc.scene_rows(drawn['val'][b])] for b in range(args.val_clips)]
    emit(dict(record='scene_training', what='setup', train_clips=args.train_clips, val_clips=args.val_clips, clip_s=args.clip_s,
              train_items=int(drawn['train'].n_items), val_items=int(drawn['val'].n_items), train_chunks=len(banks['train']), classes=NC,
              audio_format=args.format, **baffle, responses=int(rbank.n_rirs), rir_len=args.rir_len, rt60=args.rt60, events_in_pool=len(pool), **noise_rec,
              seconds_to_render_extract_and_bank=round(time.perf_counter() - t0, 2), device=torch.cuda.get_device_name(0), **room_rec,
              **(dict(moving=args.moving, traj_step=int(drawn['train'].traj_step), speed_deg_s=[10.0, 40.0],
                      train_moving_items=int((np.diff(drawn['train'].traj_start) > 0).sum()), train_trajectory_nodes=len(drawn['train'].traj_rir),
                      val_moving_items=int((np.diff(drawn['val'].traj_start) > 0).sum()),
                      val_rows_whose_direction_differs_from_the_items_first=int(sum(
                          (sc.scene_rows(drawn['val'][b])[:, 3] != sc.scene_rows(static_view(drawn['val'][b]))[:, 3]).sum()
                          for b in range(args.val_clips)))) if args.moving else {}),
              **(dict(n_conformer_layers=args.conformer) if args.conformer else {})))
    tr = Trainer('cuda', seed=args.seed, n_conformer_layers=args.conformer)
    keys = ('valER', 'valF1', 'valLE', 'valLR', 'valSeld')
    before = validate(tr, banks['val'], val_gt)
    emit(dict(record='scene_training', what='held-out scores before training', **{k: round(before[k], 4) for k in keys}))
    t0 = time.perf_counter()
    hist = tr.fit(banks['train'], val_bank=banks['val'], val_gt=val_gt, batch_size=args.batch, max_epochs=args.epochs, seed=args.seed,
                  audio_format=args.format)
    seconds = time.perf_counter() - t0
    steps_per_epoch = len(hist['steps']) // max(1, args.epochs)
    for v in hist['val']:
        ep = [s for s in hist['steps'] if s[0] == v['epoch']]
        emit(dict(record='scene_training', what='epoch', epoch=v['epoch'], mean_loss=round(sum(s[4] for s in ep) / len(ep), 5),
                  **{k: round(v[k], 4) for k in keys}))
    after = hist['val'][-1]
    emit(dict(record='scene_training', what='held-out scores after training', epochs=args.epochs, steps=len(hist['steps']),
              steps_per_epoch=steps_per_epoch, fit_seconds=round(seconds, 2), **{k: round(after[k], 4) for k in keys},
              valSeld_before=round(before['valSeld'], 4), best_valSeld=round(hist['best']['valSeld'], 4) if hist['best'] else None))


if __name__ == '__main__':
    main()
