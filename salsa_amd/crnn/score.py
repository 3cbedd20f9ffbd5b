"""SELD scoring of DCASE rows on the device (salsa_nn_seld_score, salsa_nn_seld_score2020 for eval_version '2020' and
salsa_nn_seld_score2022 for '2022'; include/salsa_nn.h): the int16 rows `decode_dcase_rows` leaves in device memory are scored against ground-truth rows in one launch,
per (file, 1-s segment), and ten integers, one double and a status per segment come back instead of the rows.
crnn/metrics.py::SeldMetrics (2021, the default everywhere) and SeldMetrics2020 stay the host scorers and the yardsticks; what is
computed is exactly what their `update` computes.

The device never decides a close call.  Its sin / cos / acos are not the host's bit for bit, and the metric compares a float64
arccos with `<=` against the threshold and lets scipy break ties between pairings.  So a segment in which another pairing costs
within `margin` degrees of the best, or a slot average lies within `margin` of the threshold, comes back with status 1 (doubt) and
zero counters; a (class, frame) cell with more than 4 DOAs on a side gives status 2 (refused).  `score_dcase_rows` fetches the rows
of those files and runs `SeldMetrics.update` on the rows of each such segment alone (as a file of that one segment, so nothing
else is added): the numpy + scipy semantics, exactly.  DEFAULT_MARGIN is at least 16 times the largest deviation of the device's distance
from `angular_distance_deg` over every integer (elevation, elevation, |azimuth difference|) triple, measured by
tools/probe_score_distance.py (profiles/seld_score_distance.txt).

The 2020 metric (eval_version='2020', DeviceSeldScore2020) uses only the VALUE of a frame's least pairing cost, never the pairing,
so a rival pairing is no doubt there: status 1 means a class average within `margin` of the threshold, nothing else, and the host
resolves such segments with `SeldMetrics2020.update`.

The class-wise 2022 metric (eval_version='2022', DeviceSeldScore2022) is the 2021 pairing and bookkeeping with
the class axis kept: salsa_nn_seld_score2022 writes five counters and a total_DE share per class of every segment and S, D, I per
segment, and a second kernel adds each file's scored records up in segment order.  What comes back is one record per FILE, the doubt
and refused segments are scored by `SeldMetrics2022.update` and added to THEIR file's record, so the file records -- and with them
`jackknife()` -- are the host scorer's."""
import ctypes as C

import numpy as np

from .. import _lib
from .metrics import SeldMetrics, SeldMetrics2020, SeldMetrics2022

# degrees; the worst |device distance - angular_distance_deg| over all 181 x 181 x 361 integer triples is 1.207e-6 (profiles/
# seld_score_distance.txt): 83 times that, where at least 16 is asked.  A 2020 class average is a mean over frames of sums of at most
# four distances, each within those 1.207e-6 of the host's, so the average is within 4.83e-6: the margin is 20 times that.
DEFAULT_MARGIN = 1e-4
COUNTERS = ('TP', 'FP', 'FN', 'S', 'D', 'I', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')
COUNTERS_2020 = ('TP', 'FP', 'FN', 'TN', 'S', 'D', 'I', 'Nref', 'Nsys', 'DE_TP')
CLASS_COUNTERS_2022 = ('TP', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')       # per class, as the device stores them; the rest follows from these
SCORED, DOUBT, REFUSED = 0, 1, 2


class _DeviceScore:
    """what DeviceSeldScore and DeviceSeldScore2020 add to their host scorer"""

    def __init__(self, n_classes: int = 12, doa_threshold: float = 20, label_rate: int = 10, margin: float = DEFAULT_MARGIN):
        super().__init__(n_classes, doa_threshold)
        self.label_rate, self.margin = label_rate, margin
        self.n_segments = self.n_doubt = self.n_refused = 0

    def _check_merge(self, other):
        if getattr(other, 'eval_version', None) != self.eval_version:
            raise ValueError('merge: %s into SELD %s scores' % (type(other).__name__, self.eval_version))
        if (other.n_classes, other.doa_threshold) != (self.n_classes, self.doa_threshold):
            raise ValueError('merge: scores of %d classes at %s degrees into %d classes at %s degrees'
                             % (other.n_classes, other.doa_threshold, self.n_classes, self.doa_threshold))

    def merge(self, other):
        self._check_merge(other)
        for name in self.counter_names + ('n_segments', 'n_doubt', 'n_refused'):
            setattr(self, name, getattr(self, name) + getattr(other, name, 0))
        self.total_DE += other.total_DE
        return self


class DeviceSeldScore(_DeviceScore, SeldMetrics):
    """SeldMetrics' counters, `scores()` and `seld_error()`, filled by `score_dcase_rows`; `n_segments`, `n_doubt` and `n_refused`
    count the segments scored in all and those handed to the host; `merge` adds another result (sub-batches, ranks).  label_rate
    and margin are what `infer_pipelined(score=...)` scores with when this is its accumulator."""

    counter_names, eval_version = COUNTERS, '2021'


class DeviceSeldScore2020(_DeviceScore, SeldMetrics2020):
    """DeviceSeldScore for the SELD 2020 metric: SeldMetrics2020's counters, `scores()` and `seld_error()`, filled by
    `score_dcase_rows(eval_version='2020')`.  As the accumulator of `infer_pipelined(score=...)` its TYPE selects the 2020 metric;
    merging the other version's scores into either is a ValueError."""

    counter_names, eval_version = COUNTERS_2020, '2020'


class DeviceSeldScore2022(_DeviceScore, SeldMetrics2022):
    """DeviceSeldScore for the class-wise SELD 2022 metric: SeldMetrics2022's per-class counters, file records, `scores()`,
    `classwise()`, `seld_error()` and `jackknife()`, filled by `score_dcase_rows(eval_version='2022')`.  As the accumulator of
    `infer_pipelined(score=...)` its TYPE selects the metric and its `average` the figure; `merge` adds the counters and appends the
    other's file records (sub-batches and ranks, in the order they are merged)."""

    eval_version = '2022'

    def __init__(self, n_classes: int = 12, doa_threshold: float = 20, label_rate: int = 10, margin: float = DEFAULT_MARGIN,
                 average: str = 'macro'):
        _DeviceScore.__init__(self, n_classes, doa_threshold, label_rate, margin)
        if average not in ('macro', 'micro'):
            raise ValueError('average must be macro or micro, not {!r}'.format(average))
        self.average = average

    def merge(self, other):
        self._check_merge(other)
        SeldMetrics2022.merge(self, other)
        for name in ('n_segments', 'n_doubt', 'n_refused'):
            setattr(self, name, getattr(self, name) + getattr(other, name, 0))
        return self


_VERSIONS = {'2021': (DeviceSeldScore, SeldMetrics, 'salsa_nn_seld_score'), '2020': (DeviceSeldScore2020, SeldMetrics2020, 'salsa_nn_seld_score2020'),
             '2022': (DeviceSeldScore2022, SeldMetrics2022, 'salsa_nn_seld_score2022')}


def _version(eval_version):
    if eval_version not in _VERSIONS:
        raise ValueError('Unknown eval_version {}'.format(eval_version))
    return _VERSIONS[eval_version]


def segment_rows_of(rows, segment: int, label_rate: int):
    """the rows (frame, class, azimuth, elevation, ...) whose frame lies in `segment`"""
    return [r for r in rows if segment * label_rate <= r[0] < (segment + 1) * label_rate]


def segment_alone(rows, segment: int, label_rate: int):
    """`segment` of a file as a file of that one segment: its rows with the frames counted from the segment's start.  Scored with
    max_frames = label_rate it adds the segment's share and nothing else (the 2020 metric books every class of an EMPTY segment as a
    true negative, so the segment's rows in a file of full length would add those of all the other segments again)."""
    return [(r[0] - segment * label_rate,) + tuple(r[1:]) for r in segment_rows_of(rows, segment, label_rate)]


def resolve_records(sum_counters, sum_de, status, fetch_file, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                    doa_threshold: float = 20, margin: float = DEFAULT_MARGIN, eval_version: str = '2021', sum_sdi=None,
                    average: str = 'macro') -> DeviceSeldScore:
    """The host's half of `score_dcase_rows`: sum_counters (10,) and sum_de, the status-0 records added up; status (n_files, n_seg);
    fetch_file(f) -> (pred rows, gt rows) of file f as row lists, called once per file that has a segment of status 1 or 2.  Those
    segments are scored by SeldMetrics.update (eval_version '2020': SeldMetrics2020.update, -> DeviceSeldScore2020) on their own
    rows, each as a file of one segment (segment_alone), in record order.
    eval_version '2022': sum_counters (n_files, n_classes, 5) (CLASS_COUNTERS_2022), sum_de (n_files, n_classes) and sum_sdi
    (n_files, 3) are the status-0 records added up per FILE; every file becomes one file record of the DeviceSeldScore2022 (with the
    given `average`), and a doubt / refused segment, scored by SeldMetrics2022.update, is added to its own file's record."""
    result_cls, host_cls, _ = _version(eval_version)
    if eval_version == '2022':
        return _resolve_records2022(sum_counters, sum_de, sum_sdi, status, fetch_file, label_rate, n_classes, doa_threshold, margin, average)
    out = result_cls(n_classes, doa_threshold, label_rate, margin)
    for name, v in zip(out.counter_names, sum_counters):
        setattr(out, name, int(v))
    out.total_DE = float(sum_de)
    status = np.asarray(status)
    out.n_segments = int(status.size)
    out.n_doubt, out.n_refused = int((status == DOUBT).sum()), int((status == REFUSED).sum())
    for f in np.nonzero((status != SCORED).any(axis=1))[0]:
        pred, gt = fetch_file(int(f))
        for s in np.nonzero(status[f] != SCORED)[0]:
            m = host_cls(n_classes, doa_threshold)
            m.update(segment_alone(pred, int(s), label_rate), segment_alone(gt, int(s), label_rate), max_frames=label_rate,
                     label_rate=label_rate)
            for name in out.counter_names:
                setattr(out, name, getattr(out, name) + getattr(m, name))
            out.total_DE += m.total_DE
    return out


def _resolve_records2022(file_counters, file_de, file_sdi, status, fetch_file, label_rate, n_classes, doa_threshold, margin, average):
    out = DeviceSeldScore2022(n_classes, doa_threshold, label_rate, margin, average)
    five = np.asarray(file_counters, dtype=np.int64).reshape(-1, n_classes, len(CLASS_COUNTERS_2022))
    file_de, file_sdi = np.asarray(file_de, dtype=np.float64).reshape(-1, n_classes), np.asarray(file_sdi, dtype=np.int64).reshape(-1, 3)
    status = np.asarray(status)
    if not (five.shape[0] == file_de.shape[0] == file_sdi.shape[0] == status.shape[0]):
        raise ValueError('resolve_records: file sums of %d / %d / %d files for a status array of %d'
                         % (five.shape[0], file_de.shape[0], file_sdi.shape[0], status.shape[0]))
    TP, Nref, DE_TP, DE_FP, DE_FN = (five[:, :, k] for k in range(5))
    # SeldMetrics2022.CLASS_COUNTERS: TP FP FP_spatial FN Nref DE_TP DE_FP DE_FN, by the identities FP == DE_FP, FN == DE_FN,
    # FP_spatial == DE_TP - TP
    cls = np.stack([TP, DE_FP, DE_TP - TP, DE_FN, Nref, DE_TP, DE_FP, DE_FN], axis=2)
    out.n_segments = int(status.size)
    out.n_doubt, out.n_refused = int((status == DOUBT).sum()), int((status == REFUSED).sum())
    out._add_files(cls, file_de.copy(), file_sdi.copy())                      # (copies: the callers' buffers are pinned staging memory)
    for f in np.nonzero((status != SCORED).any(axis=1))[0]:
        pred, gt = fetch_file(int(f))
        for s in np.nonzero(status[f] != SCORED)[0]:
            m = SeldMetrics2022(n_classes, doa_threshold)
            m.update(segment_alone(pred, int(s), label_rate), segment_alone(gt, int(s), label_rate), max_frames=label_rate,
                     label_rate=label_rate)
            out._add(*m._totals(), file=int(f))
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
    """one salsa_nn_seld_score (eval_version '2020': salsa_nn_seld_score2020) launch whose totals and status array are on their way
    into pinned host memory behind an event; `result()` waits for that event only and resolves the doubt / refused segments on the host"""

    def __init__(self, pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin,
                 eval_version='2021', average='macro'):
        import torch
        export = _version(eval_version)[2]
        if average not in ('macro', 'micro'):
            raise ValueError('average must be macro or micro, not {!r}'.format(average))
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
                         margin=float(margin), eval_version=eval_version, average=average)
        n_files = pred_rows.shape[0]
        n_seg = -(-int(n_frames) // int(label_rate)) if label_rate > 0 and n_frames > 0 else 1
        status = torch.empty((n_files, n_seg), dtype=torch.int32, device=dev)
        if eval_version == '2022':                                            # per-class records and per-FILE sums (no grand total)
            nc = max(1, int(n_classes))
            counters = torch.empty((n_files * n_seg, nc, 5), dtype=torch.int32, device=dev)
            total_de = torch.empty((n_files * n_seg, nc), dtype=torch.float64, device=dev)
            sdi = torch.empty((n_files * n_seg, 3), dtype=torch.int32, device=dev)
            sums = torch.empty((n_files, nc, 5), dtype=torch.int64, device=dev)
            sum_de = torch.empty((n_files, nc), dtype=torch.float64, device=dev)
            sum_sdi = torch.empty((n_files, 3), dtype=torch.int64, device=dev)
            outputs = (counters, total_de, sdi, status, sums, sum_de, sum_sdi)
        else:
            counters = torch.empty((n_files * n_seg, 10), dtype=torch.int32, device=dev)
            total_de = torch.empty((n_files * n_seg,), dtype=torch.float64, device=dev)
            sums = torch.empty((10,), dtype=torch.int64, device=dev)
            sum_de = torch.empty((1,), dtype=torch.float64, device=dev)
            outputs = (counters, total_de, status, sums, sum_de)
        with torch.cuda.device(dev):
            rc = getattr(_lib.load(), export)(_ptr(self.pred_rows), _ptr(self.pred_counts), self.pred_rows.shape[1], _ptr(self.gt_rows),
                                              _ptr(self.gt_counts), self.gt_rows.shape[1], n_files, int(n_frames), int(label_rate),
                                              int(n_classes), float(doa_threshold), float(margin), *[_ptr(t) for t in outputs],
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if rc == _lib.E_INVAL:
                raise ValueError('%s refused %d files of %d frames at label rate %d with %d classes, capacities %d / %d, '
                                 'threshold %r, margin %r' % (export, n_files, n_frames, label_rate, n_classes, self.pred_rows.shape[1],
                                                              self.gt_rows.shape[1], doa_threshold, margin))
            if rc:
                raise RuntimeError('%s failed (%d)' % (export, rc))
            # (per-record outputs: kept for callers that want them; '2022': class counters, class total_DE, S D I, status)
            self.records = (counters, total_de, sdi, status) if eval_version == '2022' else (counters, total_de, status)
            self.host = {}
            to_host = [('sums', sums), ('sum_de', sum_de), ('status', status), ('pred_counts', self.pred_counts), ('gt_counts', self.gt_counts)]
            if eval_version == '2022':
                to_host.append(('sum_sdi', sum_sdi))
            for name, t in to_host:
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
        if self.args['eval_version'] == '2022':
            return resolve_records(h['sums'].numpy(), h['sum_de'].numpy(), h['status'].numpy(), self._fetch, sum_sdi=h['sum_sdi'].numpy(), **self.args)
        return resolve_records(h['sums'].numpy(), float(h['sum_de'][0]), h['status'].numpy(), self._fetch, **self.args)


def score_dcase_rows_async(pred_rows, pred_counts, gt_rows, gt_counts, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                           doa_threshold: float = 20, margin: float = DEFAULT_MARGIN, eval_version: str = '2021',
                           average: str = 'macro') -> PendingScore:
    """score_dcase_rows without the wait: the launch and the copies are issued on the current stream; `.result()` finishes"""
    return PendingScore(pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin, eval_version,
                        average)


def score_dcase_rows(pred_rows, pred_counts, gt_rows, gt_counts, n_frames: int = 600, label_rate: int = 10, n_classes: int = 12,
                     doa_threshold: float = 20, margin: float = DEFAULT_MARGIN, eval_version: str = '2021',
                     average: str = 'macro') -> DeviceSeldScore:
    """pred_rows (n_files, capacity, 4) int16 = (frame, class, azimuth, elevation) with pred_counts (n_files,) int32 -- what
    decode_dcase_rows returns -- against gt_rows / gt_counts in the same layout (gt_rows_to_device), CUDA tensors of one device.
    One salsa_nn_seld_score call on the current stream scores every (file, segment) and adds the undoubted records up on the device
    (integers exactly, total_DE as one float64 sum in record order); eleven totals, the status array and the counts are copied
    back.  Segments of status 1 (doubt) or 2 (refused) are scored by SeldMetrics.update on the host from their file's rows, fetched
    once per such file.  -> DeviceSeldScore with SeldMetrics' counters.  No host fallback: CPU tensors are refused.  A count above
    its slab's capacity is a ValueError (the kernel reads no row of such a file).  eval_version '2020': the SELD 2020 metric, by
    one salsa_nn_seld_score2020 call and SeldMetrics2020 -> DeviceSeldScore2020.  eval_version '2022': the class-wise SELD 2022
    metric, by one salsa_nn_seld_score2022 call (per-class records, each file's added up on the device; the per-file sums, the
    status array and the counts are copied back) and SeldMetrics2022 -> DeviceSeldScore2022 with one file record per file and the
    given `average` ('macro' | 'micro'; read by '2022' only).  Any other eval_version is a ValueError."""
    return score_dcase_rows_async(pred_rows, pred_counts, gt_rows, gt_counts, n_frames, label_rate, n_classes, doa_threshold, margin,
                                  eval_version, average).result()
