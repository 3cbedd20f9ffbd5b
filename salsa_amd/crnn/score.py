"""SELD 2021 scoring of DCASE rows on the device (salsa_nn_seld_score, include/salsa_nn.h): the int16 rows `decode_dcase_rows`
leaves in device memory are scored against ground-truth rows in one launch, per (file, 1-s segment), and ten integers, one double
and a status per segment come back instead of the rows.  crnn/metrics.py::SeldMetrics stays the host scorer, the default
everywhere and the yardstick; what is computed is exactly what its `update` computes.

The device never decides a close call.  Its sin / cos / acos are not the host's bit for bit, and the metric compares a float64
arccos with `<=` against the threshold and lets scipy break ties between pairings.  So a segment in which another pairing costs
within `margin` degrees of the best, or a slot average lies within `margin` of the threshold, comes back with status 1 (doubt) and
zero counters; a (class, frame) cell with more than 4 DOAs on a side gives status 2 (refused).  `score_dcase_rows` fetches the rows
of those files and runs `SeldMetrics.update` on the rows of each such segment alone (every other segment is empty, so nothing
else is added): the numpy + scipy semantics, exactly.  DEFAULT_MARGIN is at least 16 times the largest deviation of the device's distance
from `angular_distance_deg` over every integer (elevation, elevation, |azimuth difference|) triple, measured by
tools/probe_score_distance.py (profiles/seld_score_distance.txt)."""
import ctypes as C

import numpy as np

from .. import _lib
from .metrics import SeldMetrics

# degrees; the worst |device distance - angular_distance_deg| over all 181 x 181 x 361 integer triples is 1.207e-6 (profiles/
# seld_score_distance.txt): 83 times that, where at least 16 is asked
DEFAULT_MARGIN = 1e-4
COUNTERS = ('TP', 'FP', 'FN', 'S', 'D', 'I', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')
SCORED, DOUBT, REFUSED = 0, 1, 2


class DeviceSeldScore(SeldMetrics):
    """SeldMetrics' counters, `scores()` and `seld_error()`, filled by `score_dcase_rows`; `n_segments`, `n_doubt` and `n_refused`
    count the segments scored in all and those handed to the host; `merge` adds another result (sub-batches, ranks).  label_rate
    and margin are what `infer_pipelined(score=...)` scores with when this is its accumulator."""

    def __init__(self, n_classes: int = 12, doa_threshold: float = 20, label_rate: int = 10, margin: float = DEFAULT_MARGIN):
        super().__init__(n_classes, doa_threshold)
        self.label_rate, self.margin = label_rate, margin
        self.n_segments = self.n_doubt = self.n_refused = 0

    def merge(self, other):
        if (other.n_classes, other.doa_threshold) != (self.n_classes, self.doa_threshold):
            raise ValueError('merge: scores of %d classes at %s degrees into %d classes at %s degrees'
                             % (other.n_classes, other.doa_threshold, self.n_classes, self.doa_threshold))
        for name in COUNTERS + ('n_segments', 'n_doubt', 'n_refused'):
            setattr(self, name, getattr(self, name) + getattr(other, name, 0))
        self.total_DE += other.total_DE
        return self


def segment_rows_of(rows, segment: int, label_rate: int):
    """the rows (frame, class, azimuth, elevation, ...) whose frame lies in `segment`"""
    return [r for r in rows if segment * label_rate <= r[0] < (segment + 1) * label_rate]


def resolve_records(sum_counters, sum_de, status, fetch_file, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                    doa_threshold: float = 20, margin: float = DEFAULT_MARGIN) -> DeviceSeldScore:
    """The host's half of `score_dcase_rows`: sum_counters (10,) and sum_de, the status-0 records added up; status (n_files, n_seg);
    fetch_file(f) -> (pred rows, gt rows) of file f as row lists, called once per file that has a segment of status 1 or 2.  Those
    segments are scored by SeldMetrics.update on their own rows, in record order."""
    out = DeviceSeldScore(n_classes, doa_threshold, label_rate, margin)
    for name, v in zip(COUNTERS, sum_counters):
        setattr(out, name, int(v))
    out.total_DE = float(sum_de)
    status = np.asarray(status)
    out.n_segments = int(status.size)
    out.n_doubt, out.n_refused = int((status == DOUBT).sum()), int((status == REFUSED).sum())
    for f in np.nonzero((status != SCORED).any(axis=1))[0]:
        pred, gt = fetch_file(int(f))
        for s in np.nonzero(status[f] != SCORED)[0]:
            m = SeldMetrics(n_classes, doa_threshold)
            m.update(segment_rows_of(pred, int(s), label_rate), segment_rows_of(gt, int(s), label_rate), max_frames=n_frames,
                     label_rate=label_rate)
            for name in COUNTERS:
                setattr(out, name, getattr(out, name) + getattr(m, name))
            out.total_DE += m.total_DE
    return out


def pack_rows(list_of_row_lists):
    """host rows per file -> (rows (n_files, capacity, 4) int16 zero-padded, counts (n_files,) int32), numpy.  A row is (frame,
    class, azimuth, elevation) or, as load_dcase_csv and SeldMetrics.update have it, (frame, class, azimuth, elevation, track);
    the track is dropped (the metric ignores it).  ValueError for any other row length, a non-integer value (the device rows hold
    integer degrees) or a value outside int16."""
    files = []
    for f, rows in enumerate(list_of_row_lists):
        if len(rows) == 0:
            files.append(np.zeros((0, 4), dtype=np.int16))
            continue
        try:
            a = np.asarray(rows, dtype=np.float64)
        except (ValueError, TypeError):
            raise ValueError('file %d: rows of unequal length or non-numeric values' % f)
        if a.ndim != 2 or a.shape[1] not in (4, 5):
            raise ValueError('file %d: rows have %s columns, not 4 (frame, class, azimuth, elevation) or 5 (.., track)' % (f, a.shape[1:] or 0))
        a = a[:, :4]
        if not np.isfinite(a).all() or (a != np.rint(a)).any():
            raise ValueError('file %d: non-integer frames, classes or degrees cannot be scored on the device' % f)
        if a.min() < -32768 or a.max() > 32767:
            raise ValueError('file %d: values outside int16' % f)
        files.append(a.astype(np.int16))
    if not files:
        raise ValueError('no files')
    counts = np.array([len(a) for a in files], dtype=np.int32)
    out = np.zeros((len(files), max(1, int(counts.max())), 4), dtype=np.int16)
    for f, a in enumerate(files):
        out[f, :len(a)] = a
    return out, counts


def gt_rows_to_device(list_of_row_lists, device):
    """ground truth per file (4- or 5-column rows, see pack_rows) -> (rows (n_files, capacity, 4) int16, counts (n_files,) int32)
    tensors on `device`, the layout decode_dcase_rows writes and score_dcase_rows reads"""
    import torch
    rows, counts = pack_rows(list_of_row_lists)
    return torch.from_numpy(rows).to(device), torch.from_numpy(counts).to(device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class PendingScore:
    """one salsa_nn_seld_score launch whose totals and status array are on their way into pinned host memory behind an event;
    `result()` waits for that event only and resolves the doubt / refused segments on the host"""

    def __init__(self, pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin):
        import torch
        for name, r, c in (('pred', pred_rows, pred_counts), ('gt', gt_rows, gt_counts)):
            if not (r.is_cuda and c.is_cuda and r.device == pred_rows.device and c.device == pred_rows.device):
                raise ValueError('score_dcase_rows takes tensors on one CUDA device (the host scorer is metrics.SeldMetrics)')
            if r.dtype != torch.int16 or c.dtype != torch.int32 or r.dim() != 3 or r.shape[2] != 4 or c.dim() != 1 or c.shape[0] != r.shape[0]:
                raise ValueError('score_dcase_rows: %s rows %s %s / counts %s %s are not (files, capacity, 4) int16 / (files,) int32'
                                 % (name, tuple(r.shape), r.dtype, tuple(c.shape), c.dtype))
        if gt_rows.shape[0] != pred_rows.shape[0] or pred_rows.shape[0] == 0:
            raise ValueError('score_dcase_rows: %d predicted files, %d ground-truth files' % (pred_rows.shape[0], gt_rows.shape[0]))
        dev = pred_rows.device
        self.pred_rows, self.pred_counts = pred_rows.contiguous(), pred_counts.contiguous()
        self.gt_rows, self.gt_counts = gt_rows.contiguous(), gt_counts.contiguous()
        self.args = dict(n_frames=int(n_frames), label_rate=int(label_rate), n_classes=int(n_classes), doa_threshold=float(doa_threshold),
                         margin=float(margin))
        n_files = pred_rows.shape[0]
        n_seg = -(-int(n_frames) // int(label_rate)) if label_rate > 0 and n_frames > 0 else 1
        counters = torch.empty((n_files * n_seg, 10), dtype=torch.int32, device=dev)
        total_de = torch.empty((n_files * n_seg,), dtype=torch.float64, device=dev)
        status = torch.empty((n_files, n_seg), dtype=torch.int32, device=dev)
        sums = torch.empty((10,), dtype=torch.int64, device=dev)
        sum_de = torch.empty((1,), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().salsa_nn_seld_score(_ptr(self.pred_rows), _ptr(self.pred_counts), self.pred_rows.shape[1], _ptr(self.gt_rows),
                                                 _ptr(self.gt_counts), self.gt_rows.shape[1], n_files, int(n_frames), int(label_rate),
                                                 int(n_classes), float(doa_threshold), float(margin), _ptr(counters), _ptr(total_de),
                                                 _ptr(status), _ptr(sums), _ptr(sum_de), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == _lib.E_INVAL:
                raise ValueError('salsa_nn_seld_score refused %d files of %d frames at label rate %d with %d classes, capacities %d / %d, '
                                 'threshold %r, margin %r' % (n_files, n_frames, label_rate, n_classes, self.pred_rows.shape[1],
                                                              self.gt_rows.shape[1], doa_threshold, margin))
            if rc:
                raise RuntimeError('salsa_nn_seld_score failed (%d)' % rc)
            self.records = (counters, total_de, status)                       # (per-record outputs: kept for callers that want them)
            self.host = {}
            for name, t in (('sums', sums), ('sum_de', sum_de), ('status', status), ('pred_counts', self.pred_counts), ('gt_counts', self.gt_counts)):
                self.host[name] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                self.host[name].copy_(t, non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()

    def _fetch(self, f):
        h = self.host
        for name, n, cap in (('predicted', int(h['pred_counts'][f]), self.pred_rows.shape[1]), ('ground-truth', int(h['gt_counts'][f]), self.gt_rows.shape[1])):
            if n < 0 or n > cap:
                raise ValueError('file %d: %d %s rows in a slab of %d' % (f, n, name, cap))
        return (self.pred_rows[f, :int(h['pred_counts'][f])].cpu().tolist(), self.gt_rows[f, :int(h['gt_counts'][f])].cpu().tolist())

    def result(self) -> DeviceSeldScore:
        self.event.synchronize()
        h = self.host
        return resolve_records(h['sums'].numpy(), float(h['sum_de'][0]), h['status'].numpy(), self._fetch, **self.args)


def score_dcase_rows_async(pred_rows, pred_counts, gt_rows, gt_counts, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                           doa_threshold: float = 20, margin: float = DEFAULT_MARGIN) -> PendingScore:
    """score_dcase_rows without the wait: the launch and the copies are issued on the current stream; `.result()` finishes"""
    return PendingScore(pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin)


def score_dcase_rows(pred_rows, pred_counts, gt_rows, gt_counts, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                     doa_threshold: float = 20, margin: float = DEFAULT_MARGIN) -> DeviceSeldScore:
    """pred_rows (n_files, capacity, 4) int16 = (frame, class, azimuth, elevation) with pred_counts (n_files,) int32 -- what
    decode_dcase_rows returns -- against gt_rows / gt_counts in the same layout (gt_rows_to_device), CUDA tensors of one device.
    One salsa_nn_seld_score call on the current stream scores every (file, segment) and adds the undoubted records up on the device
    (integers exactly, total_DE as one float64 sum in record order); eleven totals, the status array and the counts are copied
    back.  Segments of status 1 (doubt) or 2 (refused) are scored by SeldMetrics.update on the host from their file's rows, fetched
    once per such file.  -> DeviceSeldScore with SeldMetrics' counters.  No host fallback: CPU tensors are refused.  A count above
    its slab's capacity is a ValueError (the kernel reads no row of such a file)."""
    return score_dcase_rows_async(pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin).result()
