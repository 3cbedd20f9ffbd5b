"""Whole training runs from a feature bank: the loop of the reference's ``make train`` (experiments/train.py:53-104 with Lightning's
fit loop, models/seld_models.py:84-108) around Trainer.train_step -- shuffled epochs from dataset.BankLoader (one salsa_bank_batch
call per step), the reference's step-indexed learning-rate / momentum schedule (utilities/learning_utils.py:17-52), validation every
``val_interval`` epochs through infer_pipelined with the rows decoded and scored on the device, the latest checkpoint and the best one
by valSeld under the reference's file names, and resuming.

Files (experiments/train.py:62-66; picked up by experiments/inference.py:49-67 -- ``startswith('epoch')``, ``int(f[6:9])``, and the second
number in a best file's name is valSeld):
    <out_dir>/checkpoint/epoch=003.ckpt                                              the latest epoch only
    <out_dir>/best/epoch=003-valSeld=0.512-valER=0.700-valF1=0.400-valLE=25.000-valLR=0.600.ckpt   mode 'crossval' only; one file
A checkpoint is a torch.save dict: ``state_dict`` under the reference's key names (checkpoint.reference_state_dict), the optimizer's
state, epoch, global_step, the history, and what a resumed run needs to repeat the uninterrupted one bit for bit -- torch's CPU and
device generator states (dropout seeds come from the CPU generator) and the loader's seed."""
import os

import numpy as np
import torch

from .checkpoint import load_reference_state_dict, reference_state_dict
from .train import LRS, MILESTONES

MOMS = (0.9, 0.9, 0.9, 0.9)


def lr_mom_at_step(step, steps_per_epoch, max_epochs, milestones=MILESTONES, lrs=LRS, moms=MOMS):
    """(lr, momentum) of global step ``step``: LearningRateScheduler's arithmetic exactly (learning_utils.py:26-27, :44-46) --
    np.interp over the INTEGER step milestones int(m * n_steps), n_steps = int(max_epochs * steps_per_epoch).  (train.lr_at
    interpolates over step / total_steps instead; the two agree at the shipped 50 x 1313 steps and differ for short runs.)"""
    n_steps = int(max_epochs * steps_per_epoch)
    step_milestones = [int(m * n_steps) for m in milestones]
    return float(np.interp(step, step_milestones, lrs)), float(np.interp(step, step_milestones, moms))


def best_name(epoch, val):
    """ModelCheckpoint's '{epoch:03d}-{valSeld:.3f}-{valER:.3f}-{valF1:.3f}-{valLE:.3f}-{valLR:.3f}' (train.py:65-66; Lightning
    writes every key as name=value)"""
    return ('epoch=%03d-valSeld=%.3f-valER=%.3f-valF1=%.3f-valLE=%.3f-valLR=%.3f.ckpt'
            % (epoch, val['valSeld'], val['valER'], val['valF1'], val['valLE'], val['valLR']))


def _ckpt_files(d):
    return sorted(f for f in os.listdir(d) if f.startswith('epoch') and f.endswith('ckpt')) if os.path.isdir(d) else []


def _rescore_kept(sweep, scorer, sed_threshold, val_gt, gt_rows, gt_counts, n_label, rate, trainer, unify_deg, on_gpu, return_rows):
    """the second half of validate(calibrate=): the combined file outputs the sweep kept, decoded at `sed_threshold` and scored into
    `scorer`, sub-batch by sub-batch in item order -- no forward.  -> the rows per clip (on the GPU only when return_rows asks for
    them: the scorer reads the rows on the device)"""
    from .calibrate import host_rows
    from .decode import _device_thresholds, decode_dcase_rows, decode_multi_rows, rows_to_list
    from .score import score_dcase_rows
    nc, fmt, rows, lo = trainer.n_classes, trainer.output_format, [], 0
    thr = _device_thresholds(sed_threshold, nc, trainer.device) if on_gpu else None      # uploaded once for all sub-batches
    for act, xyz in sweep.outputs:
        hi = lo + len(act)
        if on_gpu:
            if fmt == 'multi_accdoa':
                r, c = decode_multi_rows(act, xyz, n_frames=n_label, sed_threshold=thr, unify_deg=unify_deg, n_classes=nc)
            else:
                r, c = decode_dcase_rows(act, xyz, act.shape[1], act.shape[1], n_frames=n_label, sed_threshold=thr)
            scorer.merge(score_dcase_rows(r, c, gt_rows[lo:hi], gt_counts[lo:hi], n_frames=n_label, label_rate=rate, n_classes=nc,
                                          doa_threshold=scorer.doa_threshold, margin=scorer.margin, eval_version='2022',
                                          average=scorer.average))
            if return_rows:
                rows += rows_to_list(r.cpu(), c.cpu(), eval_version='2020')
        else:
            for i in range(lo, hi):
                rows.append(host_rows(act[i - lo], xyz[i - lo], sed_threshold, n_label, nc, fmt, unify_deg))
                scorer.update(rows[-1], val_gt[i], max_frames=n_label, label_rate=rate)
        lo = hi
    return rows


def validate(trainer, val_bank, val_gt, chunk_len=None, chunk_hop_len=None, combine_method='mean', sed_threshold=None,
             doa_threshold=20, eval_version='2021', sub_batch=8, return_rows=False, tta=None, unify_deg=15.0, track_merge=None,
             calibrate=None):
    """One validation pass (models/seld_models.py:96-108 + interfaces.py:163-180): every clip of ``val_bank`` through
    infer_pipelined(Trainer.infer) in test chunks, rows against ``val_gt`` (per clip a list of rows, metrics.load_dcase_csv).  On the
    GPU the rows are decoded and scored on the device (DeviceSeldScore / DeviceSeldScore2020 / DeviceSeldScore2022 by eval_version), on
    the CPU by the host classes.  eval_version '2022': valF1, valLE, valLR and valSeld are the class-wise (macro) figures of SeldMetrics2022.  tta = (audio_format, feature_type) or a tta.TtaForward: the forward is Trainer.infer under test-time augmentation (all
    channel-swap variants, the trainer's n_classes and output_format); None: Trainer.infer itself.  A 'multi_accdoa' trainer is
    decoded with track unification (infer_pipelined's output_format / unify_deg): whole clips or non-overlapping chunks, no tta --
    unless track_merge='align' (DESIGN.md section 9u), under which overlapping chunks and tta=, alone or together, are merged after
    their tracks are aligned cell by cell.
    sed_threshold: a scalar or one value per class; None: the trainer's calibrated ``sed_thresholds`` (set by fit(calibrate=) and by
    resuming its checkpoints), or 0.3 when it has none.
    calibrate = candidate thresholds, (K,) or (K, n_classes) (eval_version '2022' only): ONE forward pass with
    infer_pipelined(sweep=), calibrate.ThresholdSweep.best() picks a threshold per class (a class without references keeps
    sed_threshold), and the KEPT combined outputs are decoded and scored at the chosen vector -- no second forward.  The figures are
    those of validate(sed_threshold=chosen); 'thresholds' holds the chosen (n_classes,) float32 vector and 'sweep' the accumulator.
    -> dict valER valF1 valLE valLR valSeld (+ the scorer under 'scorer', and 'rows' when asked)."""
    from .infer import infer_pipelined
    from .tta import wrap_forward
    from .metrics import SeldMetrics, SeldMetrics2020, SeldMetrics2022
    from .score import DeviceSeldScore, DeviceSeldScore2020, DeviceSeldScore2022, gt_rows_to_device
    if eval_version not in ('2020', '2021', '2022'):
        raise ValueError('Unknown eval_version {}'.format(eval_version))
    device_cls, host_cls = {'2020': (DeviceSeldScore2020, SeldMetrics2020), '2021': (DeviceSeldScore, SeldMetrics),
                            '2022': (DeviceSeldScore2022, SeldMetrics2022)}[eval_version]
    if calibrate is not None and eval_version != '2022':
        raise ValueError("calibrate= tunes the class-wise metric: it needs eval_version='2022', not {!r}".format(eval_version))
    if sed_threshold is None:
        sed_threshold = getattr(trainer, 'sed_thresholds', None)
        sed_threshold = 0.3 if sed_threshold is None else sed_threshold
    n = len(val_bank.clip_len)
    if n == 0 or len(val_gt) != n:
        raise ValueError('validation: ground truth of %d clips for a bank of %d' % (len(val_gt), n))
    if len(set(val_bank.clip_len)) != 1:
        raise ValueError('validation: clips of unequal length in the bank: %s frames' % sorted(set(val_bank.clip_len)))
    n_label = val_bank.clip_len[0] // val_bank.upsample
    nc, rate = trainer.n_classes, val_bank.label_rate
    on_gpu = trainer.device.type == 'cuda'
    forward = wrap_forward(trainer.infer, tta, nc, trainer.output_format, track_merge)
    kw = dict(sub_batch=sub_batch, sed_threshold=sed_threshold, n_label_frames=n_label, chunk_len=chunk_len, chunk_hop_len=chunk_hop_len,
              combine_method=combine_method, n_classes=nc, output_format=trainer.output_format, unify_deg=unify_deg,
              track_merge=track_merge, eval_version='2020')       # (the ROW shape only: (frame, class, azimuth, elevation), what SeldMetrics.update reads)
    scorer = device_cls(nc, doa_threshold, rate) if on_gpu else host_cls(nc, doa_threshold)
    gt_rows, gt_counts = gt_rows_to_device(val_gt, trainer.device) if on_gpu else (None, None)
    chosen = sweep = None
    if calibrate is not None:
        from .calibrate import ThresholdSweep
        sweep = ThresholdSweep(calibrate, nc, doa_threshold, rate)
        infer_pipelined(n, val_bank.clip_batch, forward, decode='device' if on_gpu else 'host',
                        sweep=(gt_rows, gt_counts, sweep) if on_gpu else (val_gt, None, sweep), return_rows=False, **kw)   # (no rows yet: no threshold yet)
        chosen = sweep.best(default=sed_threshold)[0]
        rows = _rescore_kept(sweep, scorer, chosen, val_gt, gt_rows, gt_counts, n_label, rate, trainer, unify_deg, on_gpu, return_rows)
        sweep.outputs = []                                                       # (the outputs have served: a clip's worth of floats each)
    elif on_gpu:
        rows = infer_pipelined(n, val_bank.clip_batch, forward, decode='device', score=(gt_rows, gt_counts, scorer), **kw)
    else:
        rows = infer_pipelined(n, val_bank.clip_batch, forward, decode='host', **kw)
        for pred, gt in zip(rows, val_gt):
            scorer.update(pred, gt, max_frames=n_label, label_rate=rate)
    ER, F, LE, LR = (float(v) for v in scorer.scores())
    out = dict(valER=ER, valF1=F, valLE=LE, valLR=LR, valSeld=float(scorer.seld_error()), scorer=scorer)
    if calibrate is not None:
        out.update(thresholds=chosen, sweep=sweep)
    if return_rows:
        out['rows'] = rows
    return out


def _save(path, trainer, loader, epoch, global_step, history, best, val=None):
    dev = trainer.device
    ckpt = dict(state_dict=reference_state_dict(trainer.raw_model), optimizer=trainer.opt.state_dict(), epoch=epoch,
                global_step=global_step, history=history, best=best, val=val, loader_seed=loader.seed,
                output_format=trainer.output_format, n_classes=trainer.n_classes,
                n_attn_layers=trainer.n_attn_layers, n_attn_heads=trainer.n_attn_heads, **trainer.conformer,
                **({} if getattr(trainer, 'sed_thresholds', None) is None else {'sed_thresholds': np.asarray(trainer.sed_thresholds, np.float32)}),
                rng_cpu=torch.get_rng_state(), rng_device=torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None)
    tmp = path + '.tmp'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)                                                       # (a killed job never leaves half a checkpoint)


def _load(path, trainer, loader):
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    if ckpt['loader_seed'] != loader.seed:
        raise ValueError('resume: the checkpoint was trained with loader seed %d, this run has %d' % (ckpt['loader_seed'], loader.seed))
    if ckpt.get('output_format', trainer.output_format) != trainer.output_format:
        raise ValueError('resume: the checkpoint was trained with output_format %r, this trainer has %r'
                         % (ckpt['output_format'], trainer.output_format))
    # (a checkpoint from before the attention stage has neither key: it was trained without blocks)
    stored = (ckpt.get('n_attn_layers', 0), ckpt.get('n_attn_heads', trainer.n_attn_heads))
    if stored[0] != trainer.n_attn_layers or (stored[0] > 0 and stored[1] != trainer.n_attn_heads):
        raise ValueError('resume: the checkpoint was trained with n_attn_layers %d, n_attn_heads %d, this trainer has %d, %d'
                         % (stored + (trainer.n_attn_layers, trainer.n_attn_heads)))
    # (likewise a checkpoint from before the Conformer blocks; with blocks, every setting of theirs must agree)
    if ckpt.get('n_conformer_layers', 0) != trainer.conformer['n_conformer_layers']:
        raise ValueError('resume: the checkpoint was trained with n_conformer_layers %d, this trainer has %d'
                         % (ckpt.get('n_conformer_layers', 0), trainer.conformer['n_conformer_layers']))
    if trainer.conformer['n_conformer_layers'] > 0:
        for key in ('conformer_heads', 'conformer_ff', 'conformer_kernel', 'conformer_dropout'):
            if ckpt.get(key, trainer.conformer[key]) != trainer.conformer[key]:
                raise ValueError('resume: the checkpoint was trained with %s %r, this trainer has %r' % (key, ckpt[key], trainer.conformer[key]))
    load_reference_state_dict(trainer.raw_model, ckpt['state_dict'])
    trainer.opt.load_state_dict(ckpt['optimizer'])
    torch.set_rng_state(ckpt['rng_cpu'])
    if ckpt['rng_device'] is not None and trainer.device.type == 'cuda':
        torch.cuda.set_rng_state(ckpt['rng_device'], trainer.device)
    trainer.step_idx = ckpt['global_step']
    if ckpt.get('sed_thresholds') is not None:                                   # (a checkpoint of a run without calibrate= has no such key)
        trainer.sed_thresholds = np.asarray(ckpt['sed_thresholds'], dtype=np.float32)
    return ckpt


def fit(trainer, bank, val_bank=None, val_gt=None, out_dir=None, batch_size=32, max_epochs=50, epochs=None, milestones=MILESTONES,
        lrs=LRS, moms=MOMS, val_interval=1, train_fraction=1.0, audio_format='foa', feature_type='salsa', augment=True, seed=2021,
        mode='crossval', eval_version='2021', resume=False, chunk_len=None, chunk_hop_len=None, combine_method='mean',
        sed_threshold=0.3, doa_threshold=20, val_sub_batch=8, loader=None, tta=None, unify_deg=15.0, track_merge=None, calibrate=None):
    """Train ``trainer`` for ``max_epochs`` epochs of ``bank`` (a finalized GpuFeatureBank).  The keywords are the YAML's keys
    (INTEGRATION.md has the table): batch_size = training.train_batch_size; milestones / lrs / moms = training.lr_scheduler.*;
    max_epochs, val_interval = training.*; train_fraction, n_classes (Trainer's) = data.*; eval_version ('2022': valSeld, and with it
    the best checkpoint and its name, is the class-wise macro seld_error of SeldMetrics2022); mode ('crossval': the best
    checkpoint by valSeld is kept, 'eval': the latest only).  ``epochs`` caps how many epochs THIS call runs (time-sliced jobs);
    ``resume`` continues from the lexicographically last file of <out_dir>/checkpoint (train.py:37-45; none there: from scratch).
    val_bank / val_gt: the validation clips and their ground-truth rows; chunk_len .. sed_threshold, tta, unify_deg and track_merge go to the
    validation pass (validate) and to nothing else: no checkpoint stores them.  The trainer's output_format, n_attn_layers, n_attn_heads and the five Conformer settings are stored in
    every checkpoint and checked on resume; a 'multi_accdoa' trainer takes a bank of trackwise labels (GpuFeatureBank(n_classes=3 C,
    label_format='trackwise')).
    calibrate = candidate SED thresholds, (K,) or (K, n_classes), eval_version '2022' only (ValueError otherwise): every validation
    pass calibrates one threshold per class (validate(calibrate=)); the chosen vector is stored in that epoch's history['val'] entry
    ('thresholds', a list of floats), in ``trainer.sed_thresholds`` and, as 'sed_thresholds', in every checkpoint from then on; valSeld --
    and with it the best checkpoint -- is the calibrated figure.  Resuming restores ``trainer.sed_thresholds``; a checkpoint without
    the key resumes as before.  sed_threshold may itself be one value per class.
    -> the history: dict(steps=[epoch, step, lr, mom, loss, sed_loss, doa_loss per step], val=[dict per validated epoch],
    best=dict | None, epoch=epochs finished, global_step)."""
    from ..dataset import BankLoader
    if mode not in ('crossval', 'eval'):
        raise ValueError('Invalid mode {}'.format(mode))
    if (val_bank is None) != (val_gt is None):
        raise ValueError('val_bank and val_gt come together')
    if val_bank is not None and eval_version not in ('2020', '2021', '2022'):     # (what validate refuses, before an epoch is spent)
        raise ValueError('Unknown eval_version {}'.format(eval_version))
    if calibrate is not None and eval_version != '2022':
        raise ValueError("calibrate= tunes the class-wise metric: it needs eval_version='2022', not {!r}".format(eval_version))
    if val_bank is not None:
        from .tta import _check_track_merge
        _check_track_merge(track_merge, trainer.output_format)
    if val_bank is not None and len(set(val_bank.clip_len)) != 1:
        raise ValueError('validation: clips of unequal length in the bank: %s frames' % sorted(set(val_bank.clip_len)))
    if loader is None:
        loader = BankLoader(bank, batch_size=batch_size, seed=seed, audio_format=audio_format, feature_type=feature_type,
                            augment=augment, train_fraction=train_fraction)
    spe = loader.steps_per_epoch
    if spe < 1:
        raise ValueError('no training step in an epoch (train_fraction %s of %d batches)' % (train_fraction, loader.n_batches))
    ckpt_dir = os.path.join(out_dir, 'checkpoint') if out_dir is not None else None
    best_dir = os.path.join(out_dir, 'best') if out_dir is not None else None
    history = dict(steps=[], val=[], best=None, epoch=0, global_step=0)
    first_epoch = 0
    if resume:
        if out_dir is None:
            raise ValueError('resume needs out_dir')
        found = _ckpt_files(ckpt_dir)
        if found:
            ckpt = _load(os.path.join(ckpt_dir, found[-1]), trainer, loader)
            history, first_epoch = ckpt['history'], ckpt['epoch'] + 1
    last_epoch = max_epochs if epochs is None else min(max_epochs, first_epoch + epochs)
    for epoch in range(first_epoch, last_epoch):
        on_device, sched = [], []
        for step, (x, sed, doa, _) in enumerate(loader.epoch(epoch)):
            lr, mom = lr_mom_at_step(epoch * spe + step, spe, max_epochs, milestones, lrs, moms)
            on_device.append(torch.stack(trainer.train_step(x, sed, doa, lr=lr, beta1=mom)))     # (no host synchronisation in the step)
            sched.append((epoch, step, lr, mom))
        losses = torch.stack(on_device).cpu().tolist()                           # the epoch's only read-back of the losses
        history['steps'] += [s + tuple(l) for s, l in zip(sched, losses)]
        history['epoch'], history['global_step'] = epoch + 1, (epoch + 1) * spe
        val = None
        if val_bank is not None and (epoch + 1) % val_interval == 0:
            val = validate(trainer, val_bank, val_gt, chunk_len, chunk_hop_len, combine_method, sed_threshold, doa_threshold,
                           eval_version, val_sub_batch, tta=tta, unify_deg=unify_deg, track_merge=track_merge, calibrate=calibrate)
            val.pop('scorer')
            if calibrate is not None:
                val.pop('sweep')
                trainer.sed_thresholds = val['thresholds']
                val['thresholds'] = [float(t) for t in val['thresholds']]
            val['epoch'] = epoch
            history['val'].append(val)
        improved = val is not None and mode == 'crossval' and (history['best'] is None or val['valSeld'] < history['best']['valSeld'])
        if improved:
            history['best'] = dict(val)
        if out_dir is not None:
            os.makedirs(ckpt_dir, exist_ok=True)
            old = _ckpt_files(ckpt_dir)
            name = 'epoch=%03d.ckpt' % epoch
            _save(os.path.join(ckpt_dir, name), trainer, loader, epoch, history['global_step'], history, history['best'], val)
            for f in old:
                if f != name:
                    os.remove(os.path.join(ckpt_dir, f))
            if improved:
                os.makedirs(best_dir, exist_ok=True)
                old = _ckpt_files(best_dir)
                name = best_name(epoch, val)
                _save(os.path.join(best_dir, name), trainer, loader, epoch, history['global_step'], history, history['best'], val)
                for f in old:
                    if f != name:
                        os.remove(os.path.join(best_dir, f))
    return history
