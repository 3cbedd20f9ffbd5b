#!/usr/bin/env python
"""Golden vector g28 for test-time chunks (reference data.test_chunk_len_s / test_chunk_hop_len_s; models/interfaces.py:97-139
combine_chunks, :210-258 write_classwise_output_to_file, output_format 'reg_xyz'): the rows the reference writes for one file cut
into overlapping test chunks, read back from its CSV as an int16 array, for five cases in label frames (chunk_len, hop):
  exact    (160, 120) 12 classes, 2021: the chunks tile the 600 frames exactly, neighbours overlap by 40
  leftover (160, 100) 12 classes, 2021: a leftover chunk flush with the end
  triple   (160,  60) 12 classes, 2021: frames under three chunks (weights 1/4, 1/4, 1/2)
  file     (600, 600) 12 classes, 2021: one chunk, the whole file
  y2020    (160, 100) 14 classes, 2020: four columns, no track column
Inputs (tests regenerate them from the seeds in `meta`): event logits N(LOGIT_MEAN, 1) so that about 10 % of the combined
activities pass the 0.3 threshold after torch.sigmoid on the CPU (the reference's own call), xyz = tanh of normal draws.
The tool also computes every active pair's angles in float64 and asserts that at most 0.1 % of them lie within 1e-4 degrees of a
rounding boundary (the share is recorded in `meta`): outside that band the reference's float32 numpy expression and float64
arithmetic round alike.  Build-container only (needs the reference)."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

ref_shims.install()
pl = types.ModuleType('pytorch_lightning')
pl.LightningModule = torch.nn.Module
sys.modules.setdefault('pytorch_lightning', pl)
ipy = types.ModuleType('IPython')
ipy.embed = lambda *a, **k: None
sys.modules.setdefault('IPython', ipy)

from models.interfaces import BaseModel  # noqa: E402  (reference)

from salsa_amd.crnn.decode import chunk_starts  # noqa: E402

N_FRAMES, LOGIT_MEAN, BAND_DEG, BAND_CAP = 600, -2.13, 1e-4, 1e-3
CASES = (('exact', 160, 120, 12, '2021', 41), ('leftover', 160, 100, 12, '2021', 42), ('triple', 160, 60, 12, '2021', 43),
         ('file', 600, 600, 12, '2021', 44), ('y2020', 160, 100, 14, '2020', 45))


def stand_in(nc, eval_version, chunk_len, chunk_hop):
    """the attributes and methods of BaseModel the row writer reads, on a plain namespace (as g16 / g24 / g25 do)"""
    cols = ['frame_idx', 'event', 'track_number', 'azimuth', 'elevation'] if eval_version == '2021' else ['frame_idx', 'event', 'azimuth', 'elevation']
    s = types.SimpleNamespace(n_classes=nc, output_format='reg_xyz', sed_threshold=0.3, max_nframes_per_file=N_FRAMES,
                              eval_version=eval_version, df_columns=cols, label_rate=10, feature_rate=80, test_chunk_len=chunk_len * 8,
                              test_chunk_hop_len=chunk_hop * 8)
    for m in ('combine_chunks', 'write_classwise_output_to_file'):
        setattr(s, m, types.MethodType(getattr(BaseModel, m), s))
    return s


def chunk_inputs(seed, n_chunks, chunk_len, nc):
    """seeded event logits and xyz outputs of one file's chunks (the tests draw them the same way)"""
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(n_chunks, chunk_len, nc, generator=g) + LOGIT_MEAN
    xyz = torch.tanh(torch.randn(n_chunks, chunk_len, 3 * nc, generator=g))
    return logit, xyz


def band_share(s, sed, xyz, nc):
    """share of the active pairs whose float64 azimuth or elevation lies within BAND_DEG of a half-integer"""
    fs, fx = (s.combine_chunks(a) if a.shape[0] > 1 else a[0] for a in (sed, xyz))
    t, c = np.nonzero(fs[:N_FRAMES] >= np.float32(0.3))
    x, y, z = (fx[t, k * nc + c].astype(np.float64) for k in range(3))
    azi, ele = np.degrees(np.arctan2(y, x)), np.degrees(np.arctan2(z, np.sqrt(x ** 2 + y ** 2)))
    near = lambda a: np.abs(np.abs(a - np.floor(a)) - 0.5) <= BAND_DEG     # noqa: E731
    return len(t), float(np.mean(near(azi) | near(ele)))


arrays, meta = {}, {'n_frames': N_FRAMES, 'logit_mean': LOGIT_MEAN, 'sed_threshold': 0.3, 'band_deg': BAND_DEG, 'cases': {}}
with tempfile.TemporaryDirectory() as tmp:
    for name, cl, ch, nc, version, seed in CASES:
        n_chunks = len(chunk_starts(N_FRAMES, cl, ch))
        logit, xyz = chunk_inputs(seed, n_chunks, cl, nc)
        s = stand_in(nc, version, cl, ch)
        path = os.path.join(tmp, name + '.csv')
        s.write_classwise_output_to_file({'event_frame_logit': logit, 'doa_frame_output': xyz}, path)
        rows = np.loadtxt(path, delimiter=',', dtype=np.int64, ndmin=2)
        assert rows.shape[1] == (5 if version == '2021' else 4) and np.abs(rows).max() < 2 ** 15
        n_active, share = band_share(s, torch.sigmoid(logit).numpy(), xyz.numpy(), nc)
        assert n_active == rows.shape[0] and share <= BAND_CAP, (name, n_active, rows.shape, share)
        arrays['rows:%s' % name] = rows.astype(np.int16)                   # (frame < 600, class, [0,] azimuth, elevation: exact)
        meta['cases'][name] = {'chunk_len': cl, 'chunk_hop': ch, 'n_chunks': n_chunks, 'n_classes': nc, 'eval_version': version,
                               'seed': seed, 'n_rows': int(rows.shape[0]), 'band_share': share}
        print('%-8s %d chunks of %d at hop %d, %d classes: %d rows (%.1f %% active), %.3f %% of them in the rounding band'
              % (name, n_chunks, cl, ch, nc, rows.shape[0], 100.0 * rows.shape[0] / (N_FRAMES * nc), 100.0 * share))

path = os.path.join(ROOT, 'tests', 'golden', 'g28_test_chunks.npz')
np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
print(path, len(arrays), 'arrays', '%.1f KB' % (os.path.getsize(path) / 1024))
