#!/usr/bin/env python
"""Golden vector g25 for the ACCDOA output format (reference models/interfaces.py, output_format 'accdoa'):
  (a) compute_classwise_accdoa_loss on seeded inputs at (4, 80, 12) and (3, 37, 14): the doa loss (the loss compute_loss
      returns) and the autograd gradient of doa_frame_output;
  (b) get_sed_from_accdoa_output on a seeded (2, 600, 36) float32 output;
  (c) the rows write_classwise_output_to_file writes for accdoa, read back from its CSV as an int array: one whole-file
      prediction (1, 600, 36) and one chunked prediction (5 overlapping chunks of 160 label frames, hop 120), stored as int16;
  (d) one training case: the reference SeldDecoder (bigru, avg) in train() with every dropout off on a seeded (2, 512, 12, 12)
      input, compute_loss with output_format 'accdoa', backward -- the loss, stride-sampled gradients of x_fc_2.weight,
      gru.weight_hh_l1 and x_fc_1.bias, the input's gradient, and the names of the parameters whose gradient is None.
Build-container only (needs the reference)."""
import json
import logging
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

import torch.nn.functional as F  # noqa: E402

from models.decoders import SeldDecoder  # noqa: E402  (reference)
from models.interfaces import BaseModel  # noqa: E402  (reference)

from salsa_amd.crnn.model import Decoder  # noqa: E402
from salsa_amd.crnn.testing import name_map, seeded_fill  # noqa: E402

logging.getLogger('lightning').setLevel(logging.ERROR)
LOSS_SHAPES = ((4, 80, 12), (3, 37, 14))
LOSS_SEED, SED_SEED, ROWS_SEED, WEIGHT_SEED, DEC_INPUT_SEED, TRAIN_SEED = 31, 32, 33, 7, 24, 34
SED_SHAPE, DEC_SHAPE = (2, 600, 36), (2, 512, 12, 12)
CHUNK_LEN, CHUNK_HOP, N_CHUNKS = 160, 120, 5          # label frames (feature frames: x 8)


def stand_in(nc, **kw):
    """the attributes and methods of BaseModel the accdoa paths read, on a plain namespace (as g16 / g24 do)"""
    s = types.SimpleNamespace(n_classes=nc, output_format='accdoa', sed_threshold=0.3, max_nframes_per_file=600, eval_version='2021',
                              df_columns=['frame_idx', 'event', 'track_number', 'azimuth', 'elevation'], label_rate=10,
                              feature_rate=80, **kw)
    for m in ('compute_loss', 'compute_classwise_accdoa_loss', 'get_sed_from_accdoa_output', 'combine_chunks',
              'write_classwise_output_to_file'):
        setattr(s, m, types.MethodType(getattr(BaseModel, m), s))
    return s


def loss_inputs(shape, seed):
    """seeded predictions (tanh range), labels (activity 0.3) and unit-vector targets where active"""
    B, T, nc = shape
    g = torch.Generator().manual_seed(seed)
    pred = torch.tanh(torch.randn(B, T, 3 * nc, generator=g))
    sed = (torch.rand(B, T, nc, generator=g) < 0.3).float()
    v = torch.randn(B, T, 3, nc, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    return pred, sed, (v * sed[:, :, None, :]).reshape(B, T, 3 * nc)


def accdoa_output(shape, g):
    """xyz outputs whose per-class lengths straddle the 0.3 threshold: random directions, lengths U(0, 0.6)"""
    n, T, c3 = shape
    v = torch.randn(n, T, 3, c3 // 3, generator=g)
    v = v / v.norm(dim=2, keepdim=True) * 0.6 * torch.rand(n, T, 1, c3 // 3, generator=g)
    return v.reshape(n, T, c3).numpy().astype(np.float32)


arrays, meta = {}, {'loss_shapes': [list(s) for s in LOSS_SHAPES], 'loss_seed': LOSS_SEED, 'sed_seed': SED_SEED,
                    'sed_shape': list(SED_SHAPE), 'rows_seed': ROWS_SEED, 'chunk_len': CHUNK_LEN, 'chunk_hop': CHUNK_HOP,
                    'n_chunks': N_CHUNKS, 'weight_seed': WEIGHT_SEED, 'decoder_input_seed': DEC_INPUT_SEED,
                    'decoder_input_shape': list(DEC_SHAPE), 'train_seed': TRAIN_SEED, 'grad_strides': {}}

# (a) the loss and the gradient of the prediction
for shape in LOSS_SHAPES:
    pred, sed, doa_gt = loss_inputs(shape, LOSS_SEED)
    pred.requires_grad_(True)
    s = stand_in(shape[2])
    loss, sed_loss, doa_loss = s.compute_loss({'event_frame_gt': sed, 'doa_frame_gt': doa_gt},
                                              {'event_frame_logit': None, 'doa_frame_output': pred})
    assert sed_loss == 0.0 and float(loss) == float(doa_loss)
    loss.backward()
    key = 'loss:%dx%dx%d' % shape
    arrays[key + ':loss'] = np.array([loss.item()], dtype=np.float32)
    arrays[key + ':grad'] = pred.grad.numpy()
    print(key, float(loss))

# (b) SED from the xyz output, numpy float32
y = accdoa_output(SED_SHAPE, torch.Generator().manual_seed(SED_SEED))
arrays['sed:out'] = stand_in(12).get_sed_from_accdoa_output(y)
assert arrays['sed:out'].dtype == np.float32

# (c) DCASE rows written for accdoa: whole file and overlapping chunks
g = torch.Generator().manual_seed(ROWS_SEED)
with tempfile.TemporaryDirectory() as tmp:
    for case, shape in (('file', (1, 600, 36)), ('chunks', (N_CHUNKS, CHUNK_LEN, 36))):
        doa = accdoa_output(shape, g)
        s = stand_in(12, test_chunk_len=CHUNK_LEN * 8, test_chunk_hop_len=CHUNK_HOP * 8)
        path = os.path.join(tmp, case + '.csv')
        s.write_classwise_output_to_file({'event_frame_logit': torch.zeros(shape[0], shape[1], 12),
                                          'doa_frame_output': torch.from_numpy(doa)}, path)
        rows = np.loadtxt(path, delimiter=',', dtype=np.int64, ndmin=2)
        assert np.abs(rows).max() < 2 ** 15
        arrays['rows:%s' % case] = rows.astype(np.int16)         # (frame < 600, class, 0, azimuth, elevation: int16 is exact)
        print(case, rows.shape)

# (d) training: the reference decoder with the accdoa loss
mine = Decoder(512, 12, 256, 'bigru', 'avg')
seeded_fill(mine, WEIGHT_SEED)
ref = SeldDecoder(n_output_channels=512, n_classes=12, output_format='accdoa', decoder_type='bigru', freq_pool='avg', decoder_size=256)
ref.load_state_dict({name_map('decoder.' + k)[len('decoder.'):]: v for k, v in mine.state_dict().items()}, strict=True)
ref.train()
for m in ref.modules():
    if isinstance(m, torch.nn.Dropout):
        m.p = 0.0
    if isinstance(m, torch.nn.RNNBase):
        m.dropout = 0.0
g = torch.Generator().manual_seed(TRAIN_SEED)
sed = (torch.rand(2, 12, 12, generator=g) < 0.2).float()
v = torch.randn(2, 12, 3, 12, generator=g)
v = v / v.norm(dim=2, keepdim=True)
doa_gt = (v * sed[:, :, None, :]).reshape(2, 12, 36)
x_dec = torch.randn(*DEC_SHAPE, generator=torch.Generator().manual_seed(DEC_INPUT_SEED))
_real_dropout = F.dropout
F.dropout = lambda x, p=0.5, training=True, inplace=False: x
try:
    xi = x_dec.clone().requires_grad_(True)
    out = ref(xi)
    loss, sed_loss, doa_loss = stand_in(12).compute_loss({'event_frame_gt': sed, 'doa_frame_gt': doa_gt}, out)
    loss.backward()
finally:
    F.dropout = _real_dropout
arrays['train:loss'] = np.array([loss.item()])
arrays['train:grad:input'] = xi.grad.numpy().reshape(-1)[::61].copy()
meta['grad_strides']['input'] = 61
params = dict(ref.named_parameters())
for k in ('x_fc_2.weight', 'gru.weight_hh_l1', 'x_fc_1.bias'):
    flat = params[k].grad.detach().reshape(-1)
    st = max(1, flat.numel() // 2048)
    arrays['train:grad:decoder.%s' % k] = flat[::st].numpy().copy()
    meta['grad_strides']['decoder.%s' % k] = st
meta['grad_none'] = sorted('decoder.' + k for k, p in params.items() if p.grad is None)
assert meta['grad_none'] == sorted('decoder.event_fc_%d.%s' % (i, w) for i in (1, 2) for w in ('weight', 'bias')), meta['grad_none']
print('train', float(loss), meta['grad_none'])

path = os.path.join(ROOT, 'tests', 'golden', 'g25_accdoa.npz')
np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
print(path, len(arrays), 'arrays', '%.1f KB' % (os.path.getsize(path) / 1024))
