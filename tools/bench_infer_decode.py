#!/usr/bin/env python
"""infer_pipelined on 32 x 60-s clips (7 x 4800 x 200 features, 600 label frames) end to end -- features on the device -> CRNN
forward -> DCASE rows on the host -- for whole clips and for 4-s test chunks at a 2-s hop (the reference Database's defaults,
29 chunks per clip), with decode='host' (float outputs copied, combine_chunks + to_dcase_rows in numpy) against decode='device'
(salsa_nn_seld_decode, int16 rows copied).  The two decode paths ALTERNATE within one process, `--reps` times each after one
untimed pass; wall time of the whole call (it ends when the last clip's rows exist on the host), the median is reported with
every sample.  One JSON line is appended to --out (default profiles/infer_decode_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from salsa_amd.crnn.decode import test_chunk_frames  # noqa: E402
from salsa_amd.crnn.infer import infer_pipelined  # noqa: E402
from salsa_amd.crnn.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--clips', type=int, default=32)
ap.add_argument('--sub-batch', type=int, default=8)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer_decode_bench.jsonl'))
args = ap.parse_args()

dev = torch.device('cuda:0')
torch.manual_seed(0)
tr = Trainer(dev, total_steps=10 ** 6)
feats = torch.randn(args.clips, 7, 4800, 200, generator=torch.Generator().manual_seed(1)).to(dev)
with torch.no_grad():
    thr = float(torch.quantile(tr.infer(feats[:2])[0].flatten()[:10 ** 6], 0.9))      # about 10 % of the pairs are active
(chunk_len, chunk_hop), _ = test_chunk_frames(4.0, 2.0)
result = {'bench': 'infer_decode', 'device': torch.cuda.get_device_name(0), 'clips': args.clips, 'sub_batch': args.sub_batch,
          'reps': args.reps, 'sed_threshold': thr, 'cases': {}}
for case, kw in (('whole_clip', {}), ('chunks_4s_hop_2s', {'chunk_len': chunk_len, 'chunk_hop_len': chunk_hop})):
    samples, n_rows = {'host': [], 'device': []}, {}
    for rep in range(args.reps + 1):
        for decode in ('host', 'device'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = infer_pipelined(args.clips, lambda lo, hi: feats[lo:hi], tr.infer, sub_batch=args.sub_batch, sed_threshold=thr,
                                   as_array=True, decode=decode, **kw)
            dt = time.perf_counter() - t0
            n_rows[decode] = sum(len(r) for r in rows)
            if rep:                                                             # (the first pass of each path is not timed)
                samples[decode].append(dt * 1e3)
    result['cases'][case] = {'rows': n_rows, **{'%s_ms' % d: {'median': statistics.median(v), 'samples': [round(x, 3) for x in v]}
                                              for d, v in samples.items()}}
    print(case, {d: round(statistics.median(v), 2) for d, v in samples.items()}, n_rows, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, 'a') as f:
    f.write(json.dumps(result) + '\n')
print(json.dumps(result))
