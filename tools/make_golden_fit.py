#!/usr/bin/env python
"""Generate tests/golden/g30_fit.npz: the UPSTREAM reference's learning-rate / momentum schedule (utilities/learning_utils.py
LearningRateScheduler, imported unmodified from the reference checkout given as --reference), driven step by step the way Lightning
drives it: on_train_start once, then on_train_batch_start(trainer, module, batch, batch_idx, dataloader_idx) for every batch of every
epoch with a stub trainer, recording the lr and the first beta it leaves in the optimizer's parameter group.  Run:
    python tools/make_golden_fit.py --reference DIR

Schedules: the shipped one (experiments/configs/seld.yml: milestones 0 / 0.1 / 0.7 / 1, lrs 3e-4 3e-4 3e-4 1e-4, constant momentum)
at 50 epochs x 1313 steps, and the same learning rates with NON-constant momenta at 3 x 3, 7 x 13 and 2 x 5 steps, where
int(milestone * n_steps) is not milestone * n_steps.  pytorch_lightning is not needed to run the callback: a stand-in module with
``Callback = object`` takes its place (the way IPython is stood in for in tools/make_golden_metrics2020.py).  Data only: arrays + JSON."""
import argparse
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MILESTONES = (0.0, 0.1, 0.7, 1.0)
LRS = (3e-4, 3e-4, 3e-4, 1e-4)
SCHEDULES = [
    dict(name='shipped_50x1313', max_epochs=50, steps_per_epoch=1313, milestones=MILESTONES, lrs=LRS, moms=(0.9, 0.9, 0.9, 0.9)),
    dict(name='short_3x3', max_epochs=3, steps_per_epoch=3, milestones=MILESTONES, lrs=LRS, moms=(0.95, 0.85, 0.9, 0.99)),
    dict(name='odd_7x13', max_epochs=7, steps_per_epoch=13, milestones=MILESTONES, lrs=LRS, moms=(0.95, 0.85, 0.9, 0.99)),
    dict(name='short_2x5', max_epochs=2, steps_per_epoch=5, milestones=(0.0, 0.45, 0.9, 1.0), lrs=(1e-4, 1e-2, 1e-3, 1e-4),
         moms=(0.9, 0.8, 0.9, 0.9)),
]


class _Logger:
    def log_metrics(self, metrics, step=None):
        pass


class _Optimizer:
    def __init__(self):
        self.param_groups = [dict(lr=None, betas=None)]


class _Trainer:
    """what the callback reads of Lightning's trainer"""

    def __init__(self):
        self.optimizers, self.logger, self.current_epoch, self.global_step = [_Optimizer()], _Logger(), 0, 0


def drive(cls, max_epochs, steps_per_epoch, milestones, lrs, moms, **_):
    cb = cls(steps_per_epoch=steps_per_epoch, max_epochs=max_epochs, milestones=milestones, lrs=lrs, moms=moms)
    tr = _Trainer()
    cb.on_train_start(tr, None)
    lr, mom = [], []
    for epoch in range(max_epochs):
        tr.current_epoch = epoch
        for batch_idx in range(steps_per_epoch):
            cb.on_train_batch_start(tr, None, None, batch_idx, 0)
            g = tr.optimizers[0].param_groups[0]
            lr.append(float(g['lr']))
            mom.append(float(g['betas'][0]))
            assert g['betas'][1] == 0.999
            tr.global_step += 1
    return np.array(lr, np.float64), np.array(mom, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='checkout of the upstream repository')
    args = ap.parse_args()
    sys.path[:0] = [args.reference]
    sys.modules.setdefault('pytorch_lightning', types.SimpleNamespace(Callback=object))   # the base class only
    from utilities.learning_utils import LearningRateScheduler
    meta, arrays = {'schedules': []}, {}
    for k, sch in enumerate(SCHEDULES):
        lr, mom = drive(LearningRateScheduler, **sch)
        meta['schedules'].append({key: (list(v) if isinstance(v, tuple) else v) for key, v in sch.items()})
        arrays['s%d_lr' % k], arrays['s%d_mom' % k] = lr, mom
        print('%-16s %6d steps  lr %.6g .. %.6g  mom %.4g .. %.4g' % (sch['name'], len(lr), lr[0], lr[-1], mom.min(), mom.max()))
    path = os.path.join(ROOT, 'tests', 'golden', 'g30_fit.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print('%s: %.1f KB, %d schedules' % (path, os.path.getsize(path) / 1024, len(SCHEDULES)))


if __name__ == '__main__':
    main()
