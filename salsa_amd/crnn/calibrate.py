"""Per-class SED thresholds calibrated on validation.  The class-wise (macro) SELD 2022 figure weighs a rare
class as much as a frequent one, and every class has its own best operating point; every class counter of SeldMetrics2022 depends on
that class's predictions alone, so K candidates per class cost K scorings, not K^C.  `ThresholdSweep` accumulates the per-file
counters of K candidates x C classes and picks a threshold per class (`best`); `sweep_host` fills it with the host decoders and
SeldMetrics2022 (the yardstick, and what decode='host' runs); `sweep_outputs` fills it from the combined file outputs on the device in
ONE salsa_nn_seld_sweep launch (include/salsa_nn.h), in which a cell is decoded and paired once and a candidate only changes the
bookkeeping.

As in crnn/score.py the device never decides a close call: an entry (file, segment, candidate, class) in which another pairing
costs within `margin` of the best, or a slot average lies within `margin` of the DOA threshold (status 1, doubt), or a reference cell
holds more than 4 DOAs (status 2, refused), comes back with zeros and is scored here by `SeldMetrics2022.update` on that segment's
rows of that class at that candidate, and added to its file's record.

SALSA_HIP_SWEEP=0 sends `sweep_outputs` to the composed path instead: K x (decode_dcase_rows | decode_multi_rows, then
score_dcase_rows(eval_version='2022')).  It is what the sweep replaces, kept for A/B measurements (tools/bench_threshold_sweep.py)."""
import ctypes as C
import os

import numpy as np

from .. import _lib
from .metrics import SeldMetrics2022
from .postprocess import cos_unify_of, multi_accdoa_rows, to_dcase_rows
from .score import DEFAULT_MARGIN, DOUBT, REFUSED, SCORED, segment_alone

MAX_K = 64                                       # csrc/seld_sweep.h
FORMATS = ('reg_xyz', 'accdoa', 'multi_accdoa')


def _eight(five):
    """(.., 5) TP Nref DE_TP DE_FP DE_FN -> (.., 8) SeldMetrics2022.CLASS_COUNTERS, by FP == DE_FP, FN == DE_FN, FP_spatial == DE_TP - TP"""
    TP, Nref, DE_TP, DE_FP, DE_FN = (five[..., k] for k in range(5))
    return np.stack([TP, DE_FP, DE_TP - TP, DE_FN, Nref, DE_TP, DE_FP, DE_FN], axis=-1)


class ThresholdSweep:
    """The accumulator of a threshold sweep.  thresholds: (K,) -- one grid for every class -- or (K, n_classes), kept as float32
    (K, n_classes), 1 <= K <= 64.  Per file: `counters` (files, K, C, 8) int64 in SeldMetrics2022.CLASS_COUNTERS' order and `total_DE`
    (files, K, C) float64 -- entry [f, k, c] is what SeldMetrics2022 books for class c of file f when class c is decoded at
    thresholds[k, c].  label_rate and margin are what `infer_pipelined(sweep=...)` sweeps with; `n_entries`, `n_doubt` and `n_refused`
    count the (file, segment, candidate, class) entries of the device path and those handed to the host; `outputs` keeps the combined
    file outputs that `infer_pipelined(sweep=...)` swept, one (act, xyz) pair per sub-batch in item order."""

    def __init__(self, thresholds, n_classes: int = 12, doa_threshold: float = 20, label_rate: int = 10, margin: float = DEFAULT_MARGIN):
        thr = np.asarray(thresholds, dtype=np.float32)
        if thr.ndim == 1:
            thr = np.repeat(thr[:, None], n_classes, axis=1)
        if thr.ndim != 2 or thr.shape[1] != n_classes or not 1 <= thr.shape[0] <= MAX_K:
            raise ValueError('thresholds %s are not (K,) or (K, %d) with 1 <= K <= %d' % (np.shape(thresholds), n_classes, MAX_K))
        self.thresholds = np.ascontiguousarray(thr)
        self.n_classes, self.doa_threshold, self.label_rate, self.margin = n_classes, doa_threshold, label_rate, margin
        K = thr.shape[0]
        self.counters = np.zeros((0, K, n_classes, 8), dtype=np.int64)
        self.total_DE = np.zeros((0, K, n_classes), dtype=np.float64)
        self.n_entries = self.n_doubt = self.n_refused = 0
        self.outputs = []

    def add_files(self, counters, total_DE):
        """appends file records: counters (n, K, C, 8) and total_DE (n, K, C)"""
        counters, total_DE = np.asarray(counters, dtype=np.int64), np.asarray(total_DE, dtype=np.float64)
        if counters.shape[1:] != self.counters.shape[1:] or total_DE.shape != counters.shape[:3]:
            raise ValueError('add_files: counters %s / total_DE %s for a sweep of %s' % (counters.shape, total_DE.shape, self.counters.shape[1:]))
        self.counters = np.concatenate([self.counters, counters])
        self.total_DE = np.concatenate([self.total_DE, total_DE])
        return self

    def merge(self, other):
        """appends another sweep's file records (sub-batches, ranks) in the order they are merged"""
        if not isinstance(other, ThresholdSweep) or (other.n_classes, other.doa_threshold) != (self.n_classes, self.doa_threshold) \
                or not np.array_equal(other.thresholds, self.thresholds, equal_nan=True):
            raise ValueError('merge: a sweep of other candidates, classes or DOA threshold')
        self.add_files(other.counters, other.total_DE)
        for name in ('n_entries', 'n_doubt', 'n_refused'):
            setattr(self, name, getattr(self, name) + getattr(other, name))
        self.outputs += other.outputs
        return self

    def classwise(self):
        """-> (K, C, 4): F_c, LE_c, LR_c by SeldMetrics2022._classwise's expressions on the counters of all files, and
        J = ((1 - F_c) + LE_c / 180 + (1 - LR_c)) / 3 -- SELD_c without ER, which is formed over all classes at once and so is no
        property of one class's threshold."""
        cls, de = self.counters.sum(axis=0), np.add.reduce(self.total_DE, axis=0)
        out = np.zeros(cls.shape[:2] + (4,), dtype=np.float64)
        for k in range(cls.shape[0]):
            out[k, :, :3] = SeldMetrics2022._classwise(cls[k], de[k], np.zeros(3, dtype=np.int64))[:, 1:4]
        out[..., 3] = ((1.0 - out[..., 0]) + out[..., 1] / 180.0 + (1.0 - out[..., 2])) / 3
        return out

    def best(self, default=0.3):
        """-> (thresholds (C,) float32, indices (C,) int64): per class the candidate of least J; among equal J the greater threshold
        value, then the lower index.  A class with Nref == 0 over all files has nothing to calibrate on: it gets `default` (a scalar
        or one value per class) and index -1."""
        J = self.classwise()[..., 3]
        K, n = self.thresholds.shape
        default = np.broadcast_to(np.asarray(default, dtype=np.float32), (n,))
        nref = self.counters[:, 0, :, 4].sum(axis=0) if K else np.zeros(n)
        chosen, index = np.array(default, dtype=np.float32), np.full(n, -1, dtype=np.int64)
        for c in range(n):
            if nref[c] == 0:
                continue
            value = [float(t) if t == t else -np.inf for t in self.thresholds[:, c]]        # (a NaN candidate loses every tie)
            index[c] = min(range(K), key=lambda k: (J[k, c], -value[k], k))
            chosen[c] = self.thresholds[index[c], c]
        return chosen, index


def _check_format(output_format):
    if output_format not in FORMATS:
        raise ValueError('invalid output_format %r' % (output_format,))
    return output_format == 'multi_accdoa'


def host_rows(act, xyz, sed_threshold, n_frames, n_classes, output_format='reg_xyz', unify_deg=15.0):
    """the host decoder of the format on one file's combined outputs -> (frame, class, azimuth, elevation) rows"""
    if _check_format(output_format):
        return multi_accdoa_rows(act, xyz, sed_threshold=sed_threshold, unify_deg=unify_deg, n_classes=n_classes,
                                 max_nframes_per_file=n_frames, eval_version='2020')
    return to_dcase_rows(act, xyz, sed_threshold=sed_threshold, n_classes=n_classes, max_nframes_per_file=n_frames, eval_version='2020')


def sweep_host(act, xyz, gt_rows, thresholds, n_frames=None, n_classes: int = 12, doa_threshold: float = 20, label_rate: int = 10,
               output_format: str = 'reg_xyz', unify_deg: float = 15.0, accumulator: ThresholdSweep = None) -> ThresholdSweep:
    """The numpy twin of `sweep_outputs`, built from the host decoders and SeldMetrics2022 alone: act (files, T, nc | 3 C) and xyz
    (files, T, 3 nc | 9 C) combined file outputs, gt_rows per file a list of rows -> the ThresholdSweep (a new one over `thresholds`,
    or `accumulator`, whose candidates, classes and thresholds are then used) with one record per file: for every candidate k the
    file is decoded at the threshold vector thresholds[k] and scored by SeldMetrics2022.update."""
    acc = accumulator if accumulator is not None else ThresholdSweep(thresholds, n_classes, doa_threshold, label_rate)
    if len(act) != len(xyz) or len(act) != len(gt_rows):
        raise ValueError('sweep_host: %d / %d file outputs for ground truth of %d files' % (len(act), len(xyz), len(gt_rows)))
    K, n = acc.thresholds.shape
    counters, de = np.zeros((len(act), K, n, 8), dtype=np.int64), np.zeros((len(act), K, n), dtype=np.float64)
    for f in range(len(act)):
        a, x = np.asarray(act[f], np.float32), np.asarray(xyz[f], np.float32)
        T = a.shape[0] if n_frames is None else n_frames
        for k in range(K):
            m = SeldMetrics2022(n, acc.doa_threshold)
            m.update(host_rows(a, x, acc.thresholds[k], T, n, output_format, unify_deg), gt_rows[f], max_frames=T, label_rate=acc.label_rate)
            counters[f, k], de[f, k] = m._totals()[:2]
    return acc.add_files(counters, de)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_outputs(act, xyz, gt_rows, gt_counts, n_frames, n_classes, multi):
    import torch
    wa, wx = (3 * n_classes, 9 * n_classes) if multi else (n_classes, 3 * n_classes)
    if act.dim() != 3 or xyz.dim() != 3 or act.shape[:2] != xyz.shape[:2] or act.shape[2] != wa or xyz.shape[2] != wx or act.shape[0] == 0:
        raise ValueError('sweep_outputs: act %s / xyz %s are not (files, frames, %d) / (.., %d)' % (tuple(act.shape), tuple(xyz.shape), wa, wx))
    if act.shape[1] < n_frames:
        raise ValueError('sweep_outputs: outputs of %d frames, n_frames = %d' % (act.shape[1], n_frames))
    for t in (act, xyz, gt_rows, gt_counts):
        if not (t.is_cuda and t.device == act.device):
            raise ValueError('sweep_outputs takes tensors on one CUDA device (the host path is calibrate.sweep_host)')
    if act.dtype != torch.float32 or xyz.dtype != torch.float32:
        raise ValueError('sweep_outputs takes float32 outputs')
    if gt_rows.dtype != torch.int16 or gt_counts.dtype != torch.int32 or gt_rows.dim() != 3 or gt_rows.shape[2] != 4 \
            or gt_counts.shape != (gt_rows.shape[0],) or gt_rows.shape[0] != act.shape[0]:
        raise ValueError('sweep_outputs: gt rows %s %s / counts %s %s are not (%d, capacity, 4) int16 / (%d,) int32'
                         % (tuple(gt_rows.shape), gt_rows.dtype, tuple(gt_counts.shape), gt_counts.dtype, act.shape[0], act.shape[0]))


class PendingSweep:
    """one salsa_nn_seld_sweep launch whose per-file sums and status array are on their way into pinned host memory behind an event;
    `result()` waits for that event only, resolves the doubt / refused entries on the host and returns the sub-batch's ThresholdSweep"""

    def __init__(self, act, xyz, gt_rows, gt_counts, thresholds, n_frames, n_classes, doa_threshold, label_rate, margin, output_format, unify_deg):
        import torch
        multi = _check_format(output_format)
        self.acc = ThresholdSweep(thresholds, n_classes, doa_threshold, label_rate, margin)       # (shapes and K: before any device call)
        _check_outputs(act, xyz, gt_rows, gt_counts, n_frames, n_classes, multi)
        cos_unify = cos_unify_of(unify_deg) if multi else 1.0
        self.act, self.xyz, self.gt_rows, self.gt_counts = act.contiguous(), xyz.contiguous(), gt_rows.contiguous(), gt_counts.contiguous()
        self.args = dict(n_frames=int(n_frames), output_format=output_format, unify_deg=unify_deg)
        dev, n_files, (K, n) = act.device, act.shape[0], self.acc.thresholds.shape
        n_seg = -(-int(n_frames) // int(label_rate)) if label_rate > 0 and n_frames > 0 else 1
        thr = self.thresholds = torch.from_numpy(self.acc.thresholds).to(dev)
        counters = torch.empty((n_files * n_seg, K, n, 5), dtype=torch.int32, device=dev)
        class_de = torch.empty((n_files * n_seg, K, n), dtype=torch.float64, device=dev)
        status = torch.empty((n_files, n_seg, K, n), dtype=torch.int32, device=dev)
        sums = torch.empty((n_files, K, n, 5), dtype=torch.int64, device=dev)
        sum_de = torch.empty((n_files, K, n), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().salsa_nn_seld_sweep(_ptr(self.act), _ptr(self.xyz), n_files, act.shape[1], int(n_frames), n, int(multi), cos_unify,
                                                 _ptr(thr), K, _ptr(self.gt_rows), _ptr(self.gt_counts), self.gt_rows.shape[1], int(label_rate),
                                                 float(doa_threshold), float(margin), _ptr(counters), _ptr(class_de), _ptr(status), _ptr(sums),
                                                 _ptr(sum_de), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == _lib.E_INVAL:
                raise ValueError('salsa_nn_seld_sweep refused: ' + _lib.last_error())
            if rc:
                raise RuntimeError('salsa_nn_seld_sweep failed (%d)' % rc)
            self.records = (counters, class_de, status)
            self.host = {}
            for name, t in (('sums', sums), ('sum_de', sum_de), ('status', status), ('gt_counts', self.gt_counts)):
                self.host[name] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                self.host[name].copy_(t, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()

    def result(self) -> ThresholdSweep:
        self.event.synchronize()
        h, acc = self.host, self.acc
        counts, cap = h['gt_counts'].numpy(), self.gt_rows.shape[1]
        if (counts < 0).any() or (counts > cap).any():
            raise ValueError('sweep_outputs: a ground-truth count outside its slab of %d rows' % cap)
        status = h['status'].numpy()
        counters, de = _eight(h['sums'].numpy()), h['sum_de'].numpy().copy()                      # (copies: pinned staging memory)
        acc.n_entries = int(status.size)
        acc.n_doubt, acc.n_refused = int((status == DOUBT).sum()), int((status == REFUSED).sum())
        rate, n, n_frames = acc.label_rate, acc.n_classes, self.args['n_frames']
        for f in np.nonzero((status != SCORED).reshape(status.shape[0], -1).any(axis=1))[0]:
            gt = self.gt_rows[f, :int(counts[f])].cpu().tolist()
            for s in np.nonzero((status[f] != SCORED).reshape(status.shape[1], -1).any(axis=1))[0]:
                lo, hi = int(s) * rate, min(int(s) * rate + rate, n_frames)
                a, x = self.act[f, lo:hi].cpu().numpy(), self.xyz[f, lo:hi].cpu().numpy()
                gt_seg = segment_alone(gt, int(s), rate)
                for k, c in zip(*np.nonzero(status[f, s] != SCORED)):
                    pred = host_rows(a, x, acc.thresholds[k], hi - lo, n, self.args['output_format'], self.args['unify_deg'])
                    m = SeldMetrics2022(n, acc.doa_threshold)
                    m.update([r for r in pred if r[1] == c], [r for r in gt_seg if r[1] == c], max_frames=rate, label_rate=rate)
                    cls, m_de, _ = m._totals()
                    counters[f, k, c] += cls[c]
                    de[f, k, c] += m_de[c]
        return acc.add_files(counters, de)


def _sweep_composed(act, xyz, gt_rows, gt_counts, acc, n_frames, output_format, unify_deg):
    """SALSA_HIP_SWEEP=0: K x (decode, then score 2022) with the entry points the sweep replaces -> acc with the files' records"""
    from .decode import decode_dcase_rows, decode_multi_rows
    from .score import score_dcase_rows
    multi = _check_format(output_format)
    _check_outputs(act, xyz, gt_rows, gt_counts, n_frames, acc.n_classes, multi)
    per_k = []
    for k in range(acc.thresholds.shape[0]):
        thr = acc.thresholds[k]
        thr = float(thr[0]) if (thr == thr[0]).all() else thr             # one grid for every class: the scalar entry points
        if multi:
            rows, counts = decode_multi_rows(act, xyz, n_frames=n_frames, sed_threshold=thr, unify_deg=unify_deg, n_classes=acc.n_classes)
        else:
            rows, counts = decode_dcase_rows(act, xyz, act.shape[1], act.shape[1], n_frames=n_frames, sed_threshold=thr)
        score = score_dcase_rows(rows, counts, gt_rows, gt_counts, n_frames=n_frames, label_rate=acc.label_rate, n_classes=acc.n_classes,
                                 doa_threshold=acc.doa_threshold, margin=acc.margin, eval_version='2022')
        rec = score.file_records()
        per_k.append((np.stack([rec[name] for name in SeldMetrics2022.CLASS_COUNTERS], axis=2), rec['total_DE']))
        acc.n_entries, acc.n_doubt, acc.n_refused = acc.n_entries + score.n_segments, acc.n_doubt + score.n_doubt, acc.n_refused + score.n_refused
    return acc.add_files(np.stack([p[0] for p in per_k], axis=1), np.stack([p[1] for p in per_k], axis=1))


def sweep_outputs_async(act, xyz, gt_rows, gt_counts, thresholds, n_frames: int = 600, n_classes: int = 12, doa_threshold: float = 20,
                        label_rate: int = 10, margin: float = DEFAULT_MARGIN, output_format: str = 'reg_xyz', unify_deg: float = 15.0):
    """sweep_outputs without the wait: the launch and the copies are issued on the current stream; `.result()` finishes.  Under
    SALSA_HIP_SWEEP=0 the composed path runs (and waits) inside `.result()`."""
    if os.environ.get('SALSA_HIP_SWEEP', '1') == '0':
        acc = ThresholdSweep(thresholds, n_classes, doa_threshold, label_rate, margin)

        class Composed:
            def result(self):
                return _sweep_composed(act, xyz, gt_rows, gt_counts, acc, int(n_frames), output_format, unify_deg)
        return Composed()
    return PendingSweep(act, xyz, gt_rows, gt_counts, thresholds, n_frames, n_classes, doa_threshold, label_rate, margin, output_format, unify_deg)


def sweep_outputs(act, xyz, gt_rows, gt_counts, thresholds, n_frames: int = 600, n_classes: int = 12, doa_threshold: float = 20,
                  label_rate: int = 10, margin: float = DEFAULT_MARGIN, output_format: str = 'reg_xyz', unify_deg: float = 15.0) -> ThresholdSweep:
    """act (files, n_in_frames, nc | 3 C) and xyz (.., 3 nc | 9 C): the COMBINED file outputs as CUDA float32 tensors -- what
    decode_dcase_rows(return_file_outputs=True) returns, what chunk_merge_multi / TtaForward give, or a whole-clip forward -- against
    gt_rows / gt_counts (score.gt_rows_to_device), for the candidates `thresholds` (K,) or (K, n_classes).  One salsa_nn_seld_sweep
    call on the current stream; the per-file sums and the status array are copied back, and the entries of status 1 (doubt) or 2
    (refused) are scored by SeldMetrics2022.update on the host from their segment's outputs, fetched once per such segment.
    -> ThresholdSweep with one record per file: what sweep_host computes (integers equal; total_DE within DE_TP x margin, the
    device's distances not being the host's bit for bit).  No host fallback: CPU tensors are refused."""
    return sweep_outputs_async(act, xyz, gt_rows, gt_counts, thresholds, n_frames, n_classes, doa_threshold, label_rate, margin,
                               output_format, unify_deg).result()
