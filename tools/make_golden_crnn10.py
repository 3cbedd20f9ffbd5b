#!/usr/bin/env python
"""Golden vector g23 for the 10-input-channel CRNN (the baseline melspecgcc / linspecgcc features, experiments/configs/seld.yml:
n_input_channels 10): salsa_amd.crnn.SeldCRNN(n_input_channels=10) filled by seeded_fill(.., 7), copied into the REFERENCE
PannResNet22(n_input_channels=10) + SeldDecoder through the product's key map, reference eval forward + interpolate on a seeded
(2, 10, 64, 128) input.  Also stores the reference model's own state-dict keys and shapes, so that a test can hold the key map
against them.  Writes only g23 (the other CRNN fixtures are not regenerated: savez archives are not byte-reproducible).
Build-container only (needs the reference)."""
import json
import logging
import os
import sys
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

from models.decoders import SeldDecoder  # noqa: E402  (reference)
from models.encoders import PannResNet22  # noqa: E402  (reference)
from models.model_utils import interpolate_tensor as ref_interp  # noqa: E402  (reference)

from salsa_amd.crnn.model import SeldCRNN  # noqa: E402
from salsa_amd.crnn.testing import name_map, seeded_fill  # noqa: E402

logging.getLogger('lightning').setLevel(logging.ERROR)
C_IN, SHAPE = 10, (2, 10, 64, 128)
mine = SeldCRNN(n_input_channels=C_IN)
seeded_fill(mine, seed=7)
enc = PannResNet22(n_input_channels=C_IN)
dec = SeldDecoder(n_output_channels=512, n_classes=12, output_format='reg_xyz', decoder_type='bigru', freq_pool='avg',
                  decoder_size=256)
ref_keys = {'encoder.' + k: list(v.shape) for k, v in enc.state_dict().items()}
ref_keys.update({'decoder.' + k: list(v.shape) for k, v in dec.state_dict().items()})
ref_sd = {name_map(k): v for k, v in mine.state_dict().items()}
enc.load_state_dict({k[len('encoder.'):]: v for k, v in ref_sd.items() if k.startswith('encoder.')}, strict=True)
dec.load_state_dict({k[len('decoder.'):]: v for k, v in ref_sd.items() if k.startswith('decoder.')}, strict=True)
enc.eval(), dec.eval()
g = torch.Generator().manual_seed(23)
x = torch.randn(*SHAPE, generator=g)
with torch.no_grad():
    out = dec(enc(x))
    ev = ref_interp(out['event_frame_logit'], ratio=16 * 10 / 80)
    doa = ref_interp(out['doa_frame_output'], ratio=16 * 10 / 80)
path = os.path.join(ROOT, 'tests', 'golden', 'g23_crnn10.npz')
meta = {'weight_seed': 7, 'input_seed': 23, 'input_shape': list(SHAPE), 'n_input_channels': C_IN, 'ref_keys': ref_keys}
np.savez_compressed(path, meta=np.array(json.dumps(meta)), event_frame_logit=ev.numpy(), doa_frame_output=doa.numpy())
print(path, ev.shape, doa.shape, float(ev.abs().mean()), float(doa.abs().mean()), '%.1f KB' % (os.path.getsize(path) / 1024))
