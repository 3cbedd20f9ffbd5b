#!/usr/bin/env python
"""Times of the SELD CRNN per decoder option (decoder_type gru | bigru | lstm | bilstm x freq_pool avg | max | avg_max): the bf16
training step (forward, backward, Adam) on a synthetic --batch x 7 x 640 x 200 batch, and the config-5 inference forward (bf16
autocast, eval) on --batch 60-s clips (7 x 4800 x 200 -> T' = 300), each timed with a device synchronise around every call.  One
JSON line per (decoder_type, freq_pool, LSTM path): median / 10th / 90th percentile / min / max.

The LSTM path is the one selected by SALSA_FUSED_LSTM when the process starts (1: the HIP scans, 0: nn.LSTM on MIOpen).  With
--unfused-leg the tool runs the lstm / bilstm decoders once more in a CHILD process started with SALSA_FUSED_LSTM=0 and a time
limit (--child-timeout): a step that does not finish in time is recorded as such ("trains": false) instead of stopping the bench.
--output-format accdoa trains with the ACCDOA loss and infers its SED decision (the default, reg_xyz, writes the records as before;
other values add an "output_format" key).

    python tools/bench_crnn_decoders.py [--steps 20] [--warmup 3] [--decoders gru,bigru,lstm,bilstm] [--pools avg,max,avg_max]
                                        [--out profiles/crnn_decoders_bench.jsonl] [--unfused-leg] [--output-format accdoa]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)


def _stats(prefix, t):
    import numpy as np
    t = np.array(t) * 1e3
    return {prefix + '_ms_median': round(float(np.median(t)), 3), prefix + '_ms_p10': round(float(np.percentile(t, 10)), 3),
            prefix + '_ms_p90': round(float(np.percentile(t, 90)), 3), prefix + '_ms_min': round(float(t.min()), 3),
            prefix + '_ms_max': round(float(t.max()), 3)}


def run(args):
    import torch
    from salsa_amd.crnn import fused_lstm
    from salsa_amd.crnn.train import Trainer, synthetic_batch
    if not torch.cuda.is_available():
        raise SystemExit('bench_crnn_decoders needs a GPU')
    dev = torch.device('cuda:0')
    lines = []
    x, sed, doa = synthetic_batch(args.batch, dev, seed=1)
    g = torch.Generator(device=dev).manual_seed(5)
    clips = torch.randn((args.batch, 7, 4800, 200), device=dev, generator=g)          # 60-s clips at 80 frames/s
    for dt in args.decoders.split(','):
        for fp in args.pools.split(','):
            tr = Trainer(dev, total_steps=10 ** 6, decoder_type=dt, freq_pool=fp, output_format=args.output_format)
            for _ in range(args.warmup):
                tr.train_step(x, sed, doa)
            torch.cuda.synchronize()
            train = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                loss = tr.train_step(x, sed, doa)[0]
                torch.cuda.synchronize()
                train.append(time.perf_counter() - t0)
            assert bool(torch.isfinite(loss)), (dt, fp)
            for _ in range(args.warmup):
                tr.infer(clips)
            torch.cuda.synchronize()
            infer = []
            for _ in range(args.infer_steps):
                t0 = time.perf_counter()
                p, _ = tr.infer(clips)
                torch.cuda.synchronize()
                infer.append(time.perf_counter() - t0)
            assert p.shape == (args.batch, 600, 12)
            rec = dict(bench='crnn_decoders', decoder_type=dt, freq_pool=fp, batch=args.batch,
                       lstm_path=('hip' if fused_lstm.FUSED_LSTM else 'nn.LSTM') if 'lstm' in dt else None,
                       train_steps=len(train), **_stats('train_step', train), train_chunks_per_s=round(args.batch / (sorted(train)[len(train) // 2]), 1),
                       infer_calls=len(infer), **_stats('infer_60s_batch', infer), loss=round(float(loss), 5), trains=True,
                       gpu=torch.cuda.get_device_name(0))
            if args.output_format != 'reg_xyz':
                rec['output_format'] = args.output_format
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del tr
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


def unfused_leg(args):
    """the lstm / bilstm decoders with SALSA_FUSED_LSTM=0, in a child process under a time limit"""
    for dt in [d for d in args.decoders.split(',') if 'lstm' in d]:
        cmd = [sys.executable, os.path.abspath(__file__), '--steps', str(args.steps), '--warmup', str(args.warmup), '--infer-steps',
               str(args.infer_steps), '--batch', str(args.batch), '--decoders', dt, '--pools', 'avg',
               '--output-format', args.output_format] + (['--out', args.out] if args.out else [])
        env = dict(os.environ, SALSA_FUSED_LSTM='0')
        try:
            rc = subprocess.run(cmd, env=env, timeout=args.child_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 'timeout'
        if rc != 0:
            rec = dict(bench='crnn_decoders', decoder_type=dt, freq_pool='avg', batch=args.batch, lstm_path='nn.LSTM', trains=False,
                       note='child process ended with %s (limit %d s)' % (rc, args.child_timeout))
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(json.dumps(rec) + '\n')
            return rc                                      # a GPU process that failed or hung: start nothing more
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='timed training steps per decoder option')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--infer-steps', type=int, default=5, help='timed inference forwards per decoder option')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--decoders', default='gru,bigru,lstm,bilstm')
    ap.add_argument('--pools', default='avg,max,avg_max')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file too')
    ap.add_argument('--unfused-leg', action='store_true', help='only the SALSA_FUSED_LSTM=0 leg (child processes)')
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--output-format', default='reg_xyz', choices=('reg_xyz', 'accdoa'), help="the YAML's data.output_format")
    args = ap.parse_args()
    if args.unfused_leg:
        sys.exit(0 if unfused_leg(args) == 0 else 1)
    run(args)


if __name__ == '__main__':
    main()
