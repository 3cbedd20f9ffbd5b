"""Batched, sharded inference (BASELINE config 5; reference test_step + write_output_submission, models/seld_models.py:
110-117, models/interfaces.py:210-258): every rank takes a contiguous range of the sorted clip list, runs
features -> CRNN forward -> sigmoid / xyz -> combine_chunks -> DCASE rows on its own GPU, and the per-clip rows are gathered
with one all_gather_object (Python lists of a few hundred integers per clip: control-plane traffic, no tensor collective on
the data path -- SURVEY.md section 8e "Batched inference: shard clips, gather results").

The per-rank engine is `infer_pipelined`: sub-batches are ISSUED `depth` deep (default 2), so while the device works on
sub-batch k + 1 the host turns sub-batch k's (600, 12) / (600, 36) outputs -- copied into pinned host slots behind a HIP event,
no device-wide synchronize anywhere -- into DCASE rows.  `stamps` receives (lo, hi, t_issue, t_rows_on_host) per sub-batch: the
true per-clip latency of config 5 (issue of a clip's sub-batch -> its rows exist on the host), measured in the run that is also
timed for throughput."""
import collections
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from ..distributed import shard_list
from .postprocess import combine_chunks, combine_chunks_multi, multi_accdoa_rows, to_dcase_rows


def _forward_chunks(feat, forward, chunk_len, chunk_hop_len, chunk_batch, sub_batch, n_label_frames):
    """one sub-batch of clips through test chunks: split -> forward on at most chunk_batch chunks at a time -> the chunk outputs as
    (files, n_chunks, Lc, .), with the label-rate chunk length and hop (models/interfaces.py:107-108)"""
    import torch
    from .decode import chunk_starts, split_test_chunks
    b, T = feat.shape[0], feat.shape[2]
    chunks = split_test_chunks(feat, chunk_len, chunk_hop_len)
    n_chunks = chunks.shape[0] // b
    if n_chunks > 1 and chunk_hop_len > chunk_len:
        raise ValueError('chunk_hop_len %d > chunk_len %d leaves frames between the %d chunks uncovered' % (chunk_hop_len, chunk_len, n_chunks))
    lab_len, lab_hop = chunk_len * n_label_frames // T, chunk_hop_len * n_label_frames // T
    if lab_len < 1 or lab_hop < 1 or (n_chunks > 1 and len(chunk_starts(n_label_frames, lab_len, lab_hop)) != n_chunks):
        raise ValueError('%d chunks of %d feature frames at hop %d do not map onto %d label frames (chunks of %d at hop %d)'
                         % (n_chunks, chunk_len, chunk_hop_len, n_label_frames, lab_len, lab_hop))
    step = chunk_batch if chunk_batch is not None else max(1, sub_batch * T // chunk_len)
    outs = [forward(chunks[i:i + step]) for i in range(0, chunks.shape[0], step)]
    prob = torch.cat([o[0].detach().float() for o in outs]) if len(outs) > 1 else outs[0][0].detach().float()
    xyz = torch.cat([o[1].detach().float() for o in outs]) if len(outs) > 1 else outs[0][1].detach().float()
    if prob.shape[1] != lab_len or xyz.shape[1] != lab_len:
        raise ValueError('forward gave %d label frames for a chunk of %d feature frames, expected %d' % (prob.shape[1], chunk_len, lab_len))
    return prob.reshape((b, n_chunks) + tuple(prob.shape[1:])), xyz.reshape((b, n_chunks) + tuple(xyz.shape[1:])), lab_len, lab_hop


def infer_pipelined(n_items: int, featurize: Callable[[int, int], 'torch.Tensor'], forward: Callable[['torch.Tensor'], tuple],
                    sub_batch: int = 32, depth: int = 2, sed_threshold: float = 0.3, n_label_frames: int = 600,
                    as_array: bool = False, stamps: Optional[list] = None, chunk_len: Optional[int] = None,
                    chunk_hop_len: Optional[int] = None, decode: str = 'host', combine_method: str = 'mean',
                    eval_version: str = '2021', n_classes: int = 12, chunk_batch: Optional[int] = None,
                    score: Optional[tuple] = None, tta=None, output_format: str = 'reg_xyz', unify_deg: float = 15.0,
                    track_merge: Optional[str] = None, sweep: Optional[tuple] = None, return_rows: bool = True) -> list:
    """featurize(lo, hi) -> feature tensor [hi - lo, 7, T, F] of items lo..hi-1 on the model's device; forward(features) ->
    (event probabilities [b, n_label_frames, 12], xyz [b, n_label_frames, 36]).  Returns the DCASE rows of every item, in
    item order.  The device is never idle waiting for the host: up to `depth` sub-batches are in flight.

    chunk_len / chunk_hop_len (FEATURE frames; decode.test_chunk_frames gives them for the reference's test_chunk_len_s /
    test_chunk_hop_len_s): every clip is cut into test chunks (decode.split_test_chunks), forward sees at most chunk_batch chunks
    at a time (default: as many as keep chunk_batch * chunk_len <= sub_batch * T, the whole-clip call's activation footprint) and
    returns [chunks, Lc, .] for them, and the chunk outputs are combined per file (combine_method 'mean' | 'gmean').
    decode = 'host': the float outputs are copied to the host and combine_chunks + to_dcase_rows run there; 'device': one
    salsa_nn_seld_decode launch on the model's stream (decode.decode_dcase_rows) and only the int16 rows and the counts are copied,
    behind the same event -- for chunks and for whole clips alike.  With none of these given the call does what it always did.

    score = (gt_rows, gt_counts, accumulator), with decode='device' only: the ground truth of all n_items items on the model's device
    (score.gt_rows_to_device) and a score.DeviceSeldScore.  Each sub-batch's rows are scored against their slice of the ground truth
    on the same stream right behind the decode launch (score.score_dcase_rows_async, with the accumulator's n_classes, threshold,
    label_rate and margin) and merged into the accumulator when the sub-batch is finished.  The rows returned are unchanged.  The
    TYPE of the accumulator selects the metric (score.DeviceSeldScore2020: the SELD 2020 one, score.DeviceSeldScore2022: the
    class-wise 2022 one, with one file record per item); eval_version only shapes the rows ('2022' rows are '2021' rows).

    tta = (audio_format, feature_type), or a ready tta.TtaForward (which carries its own forwards): test-time augmentation.  forward is
    wrapped in a TtaForward over all channel-swap variants of that recipe (n_classes as given, output_format 'reg_xyz'), so each
    forward call -- with chunks: each chunk batch -- returns the merged outputs; everything behind the forward is untouched.  None:
    forward is called as it is.

    output_format = 'multi_accdoa' (n_classes = the REAL classes C): forward returns the track activities
    (b, frames, 3 C) and xyz (b, frames, 9 C), e.g. a multi_accdoa Trainer's infer; the rows come from postprocess.multi_accdoa_rows
    (host) or decode.decode_multi_rows (device, one salsa_nn_seld_decode_multi launch) with tracks of a class closer than unify_deg
    degrees unified, so a class may hold several rows in a frame.  Whole clips, or test chunks with chunk_hop_len == chunk_len that
    tile n_label_frames exactly (reshaped to file level, no arithmetic).  The track order is not consistent between two forwards, so
    averaging track n of one with track n of another is undefined: by default (track_merge None) overlapping chunks and tta= raise
    ValueError.  score= works as before (an accumulator of C classes).  Any other output_format: forward's outputs are taken as they
    are.

    track_merge = 'align' ('multi_accdoa' only, anything else raises ValueError): two forwards are merged after
    the tracks of one are permuted, (frame, class) cell by cell, onto the other's by the permutation of least squared distance.
    tta= wraps forward in a TtaForward(output_format='multi_accdoa', track_merge='align'); several chunks per file, overlapping or
    not, go through postprocess.combine_chunks_multi (host) or decode.chunk_merge_multi (device, one salsa_nn_chunk_merge_multi
    launch) and then the decoders above; both together compose (the wrapped forward merges per chunk batch, then the chunks are
    combined).  combine_method 'gmean' with overlapping chunks raises ValueError: a geometric mean of signed components is not
    defined.  With chunk_hop_len == chunk_len, or one chunk, the rows are those of the reshape path.

    sed_threshold: a scalar, or one value per class (REAL class for 'multi_accdoa'), for either decoder (postprocess.class_thresholds).

    sweep = (gt_rows, gt_counts, accumulator), next to score= or without it: a per-class threshold sweep with a
    calibrate.ThresholdSweep, whose candidates, classes, DOA threshold, label_rate and margin are used.  decode='device': the ground
    truth on the model's device (score.gt_rows_to_device); each sub-batch's COMBINED file outputs -- behind the chunk combine, tta= and
    track_merge='align' alike -- are swept by one salsa_nn_seld_sweep launch on the same stream (calibrate.sweep_outputs_async) and
    merged into the accumulator when the sub-batch is finished.  decode='host': gt_rows is the per-item list of row lists (gt_counts is
    not read) and calibrate.sweep_host runs on the combined host outputs.  Either way the combined outputs are kept, one (act, xyz)
    pair per sub-batch, in accumulator.outputs (on the device for decode='device').  The rows returned are unchanged.

    return_rows=False (a pass made for score= or sweep= alone): no rows are copied to the host or built there and the result is a list
    of None; on the device the row decoding itself is skipped where nothing reads the rows (no score=; for the single-vector formats
    the salsa_nn_seld_decode launch stays, it is the chunk combine that writes the file outputs).  A per-class sed_threshold is checked
    here, before the first forward, and uploaded once for all sub-batches."""
    import torch
    assert depth >= 1 and sub_batch >= 1
    if output_format not in ('reg_xyz', 'accdoa', 'multi_accdoa'):
        raise ValueError('invalid output_format %r' % (output_format,))
    multi = output_format == 'multi_accdoa'
    from .tta import _check_track_merge
    _check_track_merge(track_merge, output_format)
    align = track_merge == 'align'
    overlapping = chunk_len is not None and chunk_hop_len is not None and chunk_hop_len < chunk_len
    if multi and tta is not None and not align:
        raise ValueError("output_format 'multi_accdoa' has no test-time augmentation by default: the track order differs between "
                         "forwards, so the variants cannot be averaged track by track (track_merge='align' aligns them first)")
    if multi and overlapping and not align:
        raise ValueError("output_format 'multi_accdoa' takes whole clips or non-overlapping test chunks (chunk_hop_len %d < chunk_len %d): "
                         "the track order differs between forwards, so overlaps cannot be averaged (track_merge='align' aligns them "
                         'first)' % (chunk_hop_len, chunk_len))
    if align and overlapping and combine_method == 'gmean':
        raise ValueError("combine_method 'gmean' with overlapping 'multi_accdoa' chunks: a geometric mean of signed vector components "
                         'is not defined')
    if decode not in ('host', 'device'):
        raise ValueError("decode must be 'host' or 'device', not {!r}".format(decode))
    if combine_method not in ('mean', 'gmean'):
        raise ValueError('combine method {} is unknown'.format(combine_method))
    if chunk_len is None and chunk_hop_len is not None:
        raise ValueError('chunk_hop_len without chunk_len')
    if chunk_len is not None and (chunk_len < 1 or (chunk_hop_len is not None and chunk_hop_len < 1) or (chunk_batch is not None and chunk_batch < 1)):
        raise ValueError('chunk_len, chunk_hop_len and chunk_batch must be positive')
    if score is not None:
        if decode != 'device':
            raise ValueError("score= scores the rows of decode='device'; with decode={!r} use metrics.SeldMetrics on the returned rows".format(decode))
        gt_rows, gt_counts, accumulator = score
        if gt_rows.shape[0] != n_items or gt_counts.shape[0] != n_items:
            raise ValueError('score=: ground truth of %d files for %d items' % (gt_rows.shape[0], n_items))
    if sweep is not None:
        sweep_gt, sweep_counts, sweeper = sweep
        if len(sweep_gt) != n_items or (decode == 'device' and sweep_counts.shape[0] != n_items):
            raise ValueError('sweep=: ground truth of %d files for %d items' % (len(sweep_gt), n_items))
        if sweeper.n_classes != n_classes:
            raise ValueError('sweep=: an accumulator of %d classes for n_classes = %d' % (sweeper.n_classes, n_classes))
    from .postprocess import class_thresholds
    class_thresholds(sed_threshold, n_classes)          # (a wrong length: ValueError before any forward or device call)
    device_threshold = [sed_threshold]                  # a per-class vector is replaced by its device tensor at the first device decode
    if tta is not None:
        from .tta import wrap_forward
        forward = wrap_forward(forward, tta, n_classes, output_format, track_merge) if align else wrap_forward(forward, tta, n_classes)
    results = [None] * n_items
    on_host = return_rows or (decode == 'host' and sweep is not None)     # is anything of a sub-batch read on the host?
    slots: Dict[int, dict] = {}
    pending = collections.deque()

    def finish(k, lo, hi, t_issue, lab_len, lab_hop):
        s = slots[k % depth]
        if s['event'] is not None:
            s['event'].synchronize()                     # this sub-batch's outputs are on the host (nothing else is waited for)
        if s.get('score') is not None:
            accumulator.merge(s.pop('score').result())
        if s.get('sweep') is not None:
            part = s.pop('sweep').result()
            part.outputs = [s.pop('kept')]
            sweeper.merge(part)
        if not on_host:
            pass                                         # (return_rows=False: nothing of the sub-batch was copied)
        elif decode == 'device':
            from .decode import rows_to_list
            results[lo:hi] = rows_to_list(s['rows'][:hi - lo], s['counts'][:hi - lo], eval_version=eval_version, as_array=as_array)
        else:
            p, d = s['p'][:hi - lo].numpy(), s['d'][:hi - lo].numpy()
            combined = []                                # the file-level outputs the rows are decoded from (sweep= reads them)
            for i in range(lo, hi):
                if multi:                                # file-level outputs already (chunks were reshaped, not combined) ...
                    pi, di = p[i - lo], d[i - lo]
                    if pi.ndim == 3:                     # ... or, under track_merge='align', a file's chunks: combined here
                        pi, di = combine_chunks_multi(pi, di, lab_len, lab_hop, n_frames=n_label_frames, n_classes=n_classes)
                    combined.append((pi[:n_label_frames], di[:n_label_frames]))
                    if not return_rows:
                        continue
                    results[i] = multi_accdoa_rows(pi, di, sed_threshold=sed_threshold, unify_deg=unify_deg,
                                                   n_classes=n_classes, max_nframes_per_file=n_label_frames, eval_version=eval_version,
                                                   as_array=as_array)
                    continue
                # one chunk per file (test_chunk_len = the whole clip): combine_chunks places it, as the reference does
                pi, di = (p[i - lo], d[i - lo]) if chunk_len is not None else (p[i - lo][None], d[i - lo][None])
                fp = combine_chunks(pi, lab_len, lab_hop, n_frames=n_label_frames, combine_method=combine_method)
                fd = combine_chunks(di, lab_len, lab_hop, n_frames=n_label_frames, combine_method=combine_method)
                combined.append((fp, fd))
                if return_rows:
                    results[i] = to_dcase_rows(fp, fd, sed_threshold=sed_threshold, n_classes=n_classes, max_nframes_per_file=n_label_frames,
                                               eval_version=eval_version, as_array=as_array)
            if sweep is not None:
                from .calibrate import sweep_host
                kept = (np.stack([c[0] for c in combined]), np.stack([c[1] for c in combined]))
                sweep_host(kept[0], kept[1], sweep_gt[lo:hi], None, n_frames=n_label_frames, output_format=output_format, unify_deg=unify_deg,
                           accumulator=sweeper)
                sweeper.outputs.append(kept)
        if stamps is not None:
            stamps.append((lo, hi, t_issue, time.perf_counter()))

    for k, lo in enumerate(range(0, n_items, sub_batch)):
        hi = min(n_items, lo + sub_batch)
        t_issue = time.perf_counter()
        if chunk_len is not None:
            prob, xyz, lab_len, lab_hop = _forward_chunks(featurize(lo, hi), forward, chunk_len,
                                                          chunk_hop_len if chunk_hop_len is not None else chunk_len, chunk_batch,
                                                          sub_batch, n_label_frames)
        else:
            prob, xyz = forward(featurize(lo, hi))
            prob, xyz = prob.detach().float(), xyz.detach().float()
            lab_len = lab_hop = n_label_frames
        on_gpu = prob.is_cuda
        if multi:
            if prob.dim() == 4 and align and prob.shape[1] > 1:      # several chunks: the aligned combine (device: here; host: in finish)
                if prob.shape[2:] != (lab_len, 3 * n_classes) or xyz.shape[2:] != (lab_len, 9 * n_classes):
                    raise ValueError("output_format 'multi_accdoa': forward gave %s / %s, expected (b, %d, %d) / (.., %d) per chunk"
                                     % (tuple(prob.shape[2:]), tuple(xyz.shape[2:]), lab_len, 3 * n_classes, 9 * n_classes))
                if decode == 'device':
                    from .decode import chunk_merge_multi
                    prob, xyz = chunk_merge_multi(prob, xyz, lab_len, lab_hop, n_frames=n_label_frames, n_classes=n_classes)
            elif prob.dim() == 4:                        # chunks that tile the file: (files, n_chunks, Lc, .) -> (files, n_chunks Lc, .)
                if prob.shape[1] > 1 and prob.shape[1] * lab_len != n_label_frames:
                    raise ValueError("output_format 'multi_accdoa': %d chunks of %d label frames do not tile %d label frames exactly"
                                     % (prob.shape[1], lab_len, n_label_frames))
                prob, xyz = prob.reshape(prob.shape[0], -1, prob.shape[3]), xyz.reshape(xyz.shape[0], -1, xyz.shape[3])
            if prob.dim() == 3 and (prob.shape[1] < n_label_frames or prob.shape[2] != 3 * n_classes or xyz.shape[2] != 9 * n_classes):
                raise ValueError("output_format 'multi_accdoa': forward gave %s / %s, expected (b, >= %d, %d) / (.., %d)"
                                 % (tuple(prob.shape), tuple(xyz.shape), n_label_frames, 3 * n_classes, 9 * n_classes))
        need_rows = return_rows or score is not None
        if decode == 'device' and np.ndim(device_threshold[0]) > 0 and not torch.is_tensor(device_threshold[0]):
            from .decode import _device_thresholds
            device_threshold[0] = _device_thresholds(sed_threshold, n_classes, prob.device)
        if multi and decode == 'device':
            from .decode import decode_multi_rows
            out, file_outputs = {}, (prob, xyz)
            if need_rows:
                rows, counts = decode_multi_rows(prob, xyz, n_frames=n_label_frames, sed_threshold=device_threshold[0], unify_deg=unify_deg,
                                                 n_classes=n_classes)
                out = {'rows': rows, 'counts': counts}
        elif decode == 'device':
            from .decode import decode_dcase_rows
            if chunk_len is None:                        # whole clips: one chunk of the forward's length, trimmed to n_label_frames
                lab_len = lab_hop = prob.shape[1]
            if sweep is None:
                rows, counts = decode_dcase_rows(prob, xyz, lab_len, lab_hop, n_frames=n_label_frames, sed_threshold=device_threshold[0],
                                                 combine_method=combine_method)
            else:                                        # the same launch also writes the combined file outputs the sweep reads
                rows, counts, *file_outputs = decode_dcase_rows(prob, xyz, lab_len, lab_hop, n_frames=n_label_frames, sed_threshold=device_threshold[0],
                                                                combine_method=combine_method, return_file_outputs=True)
            out = {'rows': rows, 'counts': counts}       # 8 bytes per possible row + one count per clip instead of the float outputs
        else:
            out = {'p': prob, 'd': xyz}
        if not on_host:
            out = {}                                     # nothing of this sub-batch is read on the host
        s = slots.get(k % depth)
        if s is None or any(s[n].shape[0] < hi - lo for n in out):
            s = slots[k % depth] = {n: torch.empty((hi - lo,) + tuple(t.shape[1:]), dtype=t.dtype, pin_memory=on_gpu) for n, t in out.items()}
            s['event'] = torch.cuda.Event() if on_gpu else None
        for n, t in out.items():
            s[n][:hi - lo].copy_(t, non_blocking=True)
        if s['event'] is not None:
            s['event'].record()
        if score is not None:
            from .metrics import SeldMetrics2020, SeldMetrics2022
            from .score import score_dcase_rows_async
            version = '2022' if isinstance(accumulator, SeldMetrics2022) else ('2020' if isinstance(accumulator, SeldMetrics2020) else '2021')
            s['score'] = score_dcase_rows_async(rows, counts, gt_rows[lo:hi], gt_counts[lo:hi], n_frames=n_label_frames,
                                                label_rate=accumulator.label_rate, n_classes=accumulator.n_classes,
                                                doa_threshold=accumulator.doa_threshold, margin=accumulator.margin,
                                                eval_version=version, average=getattr(accumulator, 'average', 'macro'))
        if sweep is not None and decode == 'device':
            from .calibrate import sweep_outputs_async
            s['kept'] = tuple(file_outputs)
            s['sweep'] = sweep_outputs_async(s['kept'][0], s['kept'][1], sweep_gt[lo:hi], sweep_counts[lo:hi], sweeper.thresholds,
                                             n_frames=n_label_frames, n_classes=n_classes, doa_threshold=sweeper.doa_threshold,
                                             label_rate=sweeper.label_rate, margin=sweeper.margin, output_format=output_format,
                                             unify_deg=unify_deg)
        pending.append((k, lo, hi, t_issue, lab_len, lab_hop))
        while len(pending) >= depth:                     # slot (k + 1) % depth is free again before sub-batch k + 1 is issued
            finish(*pending.popleft())
    while pending:
        finish(*pending.popleft())
    return results


def infer_clips_sharded(names: Sequence[str], featurize: Callable[[List[str]], 'torch.Tensor'],
                        forward: Callable[['torch.Tensor'], tuple], rank: int = 0, world: int = 1, sub_batch: int = 32,
                        sed_threshold: float = 0.3, n_label_frames: int = 600, gather: bool = True, depth: int = 2,
                        stamps: Optional[list] = None, chunk_len: Optional[int] = None, chunk_hop_len: Optional[int] = None,
                        decode: str = 'host', combine_method: str = 'mean', eval_version: str = '2021', n_classes: int = 12,
                        chunk_batch: Optional[int] = None, score: Optional[tuple] = None, tta=None, output_format: str = 'reg_xyz',
                        unify_deg: float = 15.0, track_merge: Optional[str] = None, sweep: Optional[tuple] = None, return_rows: bool = True) -> Dict[str, list]:
    """names: all clip names (any order; sharded over the SORTED list).  featurize(list of names) -> feature tensor
    [b, 7, T, F] on the model's device (e.g. SalsaExtractor.extract of the clips' audio with the scaler attached, cropped
    to 8 * n_label_frames frames); forward(features) -> (event probabilities [b, n_label_frames, 12], xyz [b, .., 36]), e.g.
    Trainer.infer.  Returns {clip name: DCASE rows} for ALL clips on every rank (gather=True) or for this rank's shard.
    chunk_len, chunk_hop_len, decode, combine_method, eval_version, n_classes, chunk_batch: infer_pipelined's test-chunk and
    device-decoding options, handed through.  score = (gt_rows, gt_counts, accumulator): infer_pipelined's, for THIS rank's shard
    (the ground truth of shard_list(sorted(names), rank, world), in that order); every rank's accumulator holds its shard's score,
    to be combined with DeviceSeldScore.merge.  tta, output_format, unify_deg, track_merge: infer_pipelined's, handed through; so are
    a per-class sed_threshold and sweep = (gt_rows, gt_counts, accumulator), the ground truth and the calibrate.ThresholdSweep of THIS
    rank's shard (combined with ThresholdSweep.merge), and return_rows."""
    mine = shard_list(sorted(names), rank, world)
    rows = infer_pipelined(len(mine), lambda lo, hi: featurize(mine[lo:hi]), forward, sub_batch=sub_batch, depth=depth,
                           sed_threshold=sed_threshold, n_label_frames=n_label_frames, stamps=stamps, chunk_len=chunk_len,
                           chunk_hop_len=chunk_hop_len, decode=decode, combine_method=combine_method, eval_version=eval_version,
                           n_classes=n_classes, chunk_batch=chunk_batch, score=score, tta=tta, output_format=output_format,
                           unify_deg=unify_deg, track_merge=track_merge, sweep=sweep, return_rows=return_rows)
    out = dict(zip(mine, rows))
    if gather and world > 1:
        import torch.distributed as dist
        parts = [None] * world
        dist.all_gather_object(parts, out)
        out = {k: v for part in parts for k, v in part.items()}
    return out
