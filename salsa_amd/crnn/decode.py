"""Test-time chunks (reference data.test_chunk_len_s / test_chunk_hop_len_s: dataset/database.py:27, :98-119) and the DCASE row
decoding of a batch of files on the device (salsa_nn_seld_decode, include/salsa_nn.h): the reference cuts every test clip into
overlapping chunks, runs the model on each, averages the label-rate chunk outputs back into one file prediction
(models/interfaces.py:97-139) and writes one row per active (frame, class) pair (:210-258).  `split_test_chunks` is the cut,
`decode_dcase_rows` everything behind the model in one launch, `rows_to_list` the host's view of its result -- exactly what
crnn/postprocess.py's combine_chunks + to_dcase_rows give, which stay the host path and the yardstick."""
import ctypes as C

import numpy as np

from .. import _lib
from ..dataset import get_segment_idxes, second2frame

COMBINE = {'mean': 0, 'gmean': 1}


def test_chunk_frames(test_chunk_len_s: float, test_chunk_hop_len_s: float, fs: int = 24000, hop_len: int = 300, label_rate: float = 10):
    """The YAML keys in frames -> ((chunk_len, chunk_hop_len) in feature frames, (chunk_len, chunk_hop) in label frames): the first
    as Database.second2frame gives them (dataset/database.py:56-57), the second as combine_chunks derives them from the first
    (models/interfaces.py:107-108).  (4.0, 2.0) -> ((320, 160), (40, 20)); seld.yml's (60.0, 60.1) -> ((4800, 4808), (600, 601)): a
    hop beyond the chunk length is the reference's way of asking for the whole clip in one chunk."""
    feature_rate = fs / hop_len
    feat = (second2frame(test_chunk_len_s, fs, hop_len), second2frame(test_chunk_hop_len_s, fs, hop_len))
    return feat, tuple(int(f * label_rate / feature_rate) for f in feat)


test_chunk_frames.__test__ = False       # (a product function whose name a test collector would take for a test)


def chunk_starts(n_frames: int, chunk_len: int, chunk_hop: int) -> list:
    """combine_chunks' chunk starts (models/interfaces.py:116-119); one chunk at least as long as the file starts at 0"""
    if chunk_len >= n_frames:
        return [0]
    starts = list(range(0, n_frames - chunk_len + 1, chunk_hop))
    if (n_frames - chunk_len) % chunk_hop != 0:
        starts.append(n_frames - chunk_len)
    return starts


def split_test_chunks(feat, chunk_len: int, chunk_hop_len: int):
    """feat (b, C, T, F) -> (b * n_chunks, C, chunk_len, F), file-major (all chunks of file 0, then file 1, ...), the chunks of a
    file at get_segment_idxes(T, chunk_len, chunk_hop_len, 1, 0)'s starts (regular hops plus the leftover chunk flush with the
    end): one gather on feat's device.  A single chunk that is the whole clip is returned as it is."""
    import torch
    b, ch, T, F = feat.shape
    starts, _ = get_segment_idxes(T, chunk_len, chunk_hop_len, 1, 0)
    if len(starts) == 1 and chunk_len == T:
        return feat
    t = torch.as_tensor(starts, device=feat.device)[:, None, None] + torch.arange(chunk_len, device=feat.device)   # (n, 1, L)
    bi = torch.arange(b, device=feat.device)[:, None, None, None]
    ci = torch.arange(ch, device=feat.device)[:, None]
    return feat[bi, ci, t].reshape(b * len(starts), ch, chunk_len, F)                 # (b, n, C, L, F) in one indexing kernel


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _device_thresholds(sed_threshold, n_classes, device):
    """None for a scalar sed_threshold (the scalar entry point takes it); for a sequence the (n_classes,) float32 tensor on `device`
    that the _thr entry points read -- a wrong length raises ValueError here, before any device call.  A float32 tensor already on
    `device` is taken as it is: a caller that decodes many sub-batches uploads the vector once."""
    import torch
    if torch.is_tensor(sed_threshold):                  # uploaded already (infer_pipelined and validate do it once for all sub-batches)
        if sed_threshold.shape != (n_classes,) or sed_threshold.dtype != torch.float32 or sed_threshold.device != torch.device(device):
            raise ValueError('sed_threshold: a %s %s tensor on %s for %d classes on %s'
                             % (tuple(sed_threshold.shape), sed_threshold.dtype, sed_threshold.device, n_classes, device))
        return sed_threshold.contiguous()
    if np.ndim(sed_threshold) == 0:
        return None
    from .postprocess import class_thresholds
    return torch.from_numpy(class_thresholds(sed_threshold, n_classes)).to(device)


def decode_dcase_rows(sed, xyz, chunk_len: int, chunk_hop: int, n_frames: int = 600, sed_threshold: float = 0.3,
                      combine_method: str = 'mean', return_file_outputs: bool = False):
    """sed (n_files, n_chunks, chunk_len, nc) ACTIVITIES (Trainer.infer's first output, for reg_xyz and accdoa alike) and xyz
    (n_files, n_chunks, chunk_len, 3 nc): CUDA float32 tensors at the label rate, chunk_len / chunk_hop in label frames; a 3-D
    (n_files, chunk_len, .) pair is one chunk per file.  -> rows (n_files, n_frames * nc, 4) int16 = (frame, class, azimuth,
    elevation), of which the first counts[f] of file f are written (the rest is uninitialised memory), counts (n_files,) int32, and
    with return_file_outputs the combined float32 file_sed (n_files, n_frames, nc) and file_xyz (.., 3 nc) -- what the reference's
    write_output_prediction stores.  One launch on the current stream of the tensors' device, no synchronisation; there is no
    host fallback: CPU tensors are refused (crnn/postprocess.py holds the host functions).  sed_threshold: a scalar
    (salsa_nn_seld_decode), or one value per class (salsa_nn_seld_decode_thr; postprocess.class_thresholds)."""
    import torch
    if combine_method not in COMBINE:
        raise ValueError('combine method {} is unknown'.format(combine_method))
    if sed.dim() == 3 and xyz.dim() == 3:
        sed, xyz = sed[:, None], xyz[:, None]
    if sed.dim() != 4 or xyz.dim() != 4 or sed.shape[:3] != xyz.shape[:3] or xyz.shape[3] != 3 * sed.shape[3]:
        raise ValueError('decode_dcase_rows: sed %s / xyz %s are not (files, chunks, frames, nc) / (.., 3 nc)' % (tuple(sed.shape), tuple(xyz.shape)))
    if not (sed.is_cuda and xyz.is_cuda and sed.device == xyz.device and sed.dtype == torch.float32 and xyz.dtype == torch.float32):
        raise ValueError('decode_dcase_rows takes float32 tensors on one CUDA device (the host path is postprocess.combine_chunks + to_dcase_rows)')
    n_files, n_chunks, L, nc = sed.shape
    if L != chunk_len:
        raise ValueError('decode_dcase_rows: chunks of %d frames, chunk_len = %d' % (L, chunk_len))
    if n_files == 0:
        raise ValueError('decode_dcase_rows: no files')
    sed, xyz = sed.contiguous(), xyz.contiguous()
    dev = sed.device
    thr = _device_thresholds(sed_threshold, nc, dev)
    rows = torch.empty((n_files, n_frames * nc, 4), dtype=torch.int16, device=dev)
    counts = torch.empty((n_files,), dtype=torch.int32, device=dev)
    fs = torch.empty((n_files, n_frames, nc), dtype=torch.float32, device=dev) if return_file_outputs else None
    fx = torch.empty((n_files, n_frames, 3 * nc), dtype=torch.float32, device=dev) if return_file_outputs else None
    with torch.cuda.device(dev):
        export = _lib.load().salsa_nn_seld_decode if thr is None else _lib.load().salsa_nn_seld_decode_thr
        rc = export(_ptr(sed), _ptr(xyz), n_files, n_chunks, chunk_len, chunk_hop, n_frames, nc,
                    float(sed_threshold) if thr is None else _ptr(thr), COMBINE[combine_method], _ptr(rows), _ptr(counts), _ptr(fs),
                    _ptr(fx), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == _lib.E_INVAL:
        raise ValueError('salsa_nn_seld_decode refused %d chunks of %d frames at hop %d for %d frames x %d classes (expected %d chunks)'
                         % (n_chunks, chunk_len, chunk_hop, n_frames, nc, len(chunk_starts(n_frames, chunk_len, max(1, chunk_hop)))))
    if rc:
        raise RuntimeError('salsa_nn_seld_decode failed (%d)' % rc)
    return (rows, counts, fs, fx) if return_file_outputs else (rows, counts)


def decode_multi_rows(act, xyz, n_frames: int = 600, sed_threshold: float = 0.5, unify_deg: float = 15.0, n_classes: int = 12):
    """Multi-ACCDOA file outputs on the device: act (n_files, n_in_frames, 3 C) track activities and xyz
    (n_files, n_in_frames, 9 C), CUDA float32 at the label rate, C = n_classes REAL classes, n_in_frames >= n_frames -> rows
    (n_files, 3 * n_frames * C, 4) int16 = (frame, real class, azimuth, elevation) with near-identical tracks of a class unified, of
    which the first counts[f] of file f are written, and counts (n_files,) int32 -- rows_to_list's and the scorers' input.  One
    salsa_nn_seld_decode_multi launch on the current stream, no synchronisation; CPU tensors are refused (the host function is
    postprocess.multi_accdoa_rows, whose result this equals).  sed_threshold: a scalar, or one value per REAL class, applied to
    its three tracks (salsa_nn_seld_decode_multi_thr)."""
    import torch
    from .postprocess import cos_unify_of
    cos_unify = cos_unify_of(unify_deg)
    if act.dim() != 3 or xyz.dim() != 3 or act.shape[:2] != xyz.shape[:2] or act.shape[2] != 3 * n_classes or xyz.shape[2] != 9 * n_classes:
        raise ValueError('decode_multi_rows: act %s / xyz %s are not (files, frames, %d) / (.., %d)'
                         % (tuple(act.shape), tuple(xyz.shape), 3 * n_classes, 9 * n_classes))
    if not (act.is_cuda and xyz.is_cuda and act.device == xyz.device and act.dtype == torch.float32 and xyz.dtype == torch.float32):
        raise ValueError('decode_multi_rows takes float32 tensors on one CUDA device (the host path is postprocess.multi_accdoa_rows)')
    n_files, n_in = act.shape[:2]
    if n_files == 0:
        raise ValueError('decode_multi_rows: no files')
    act, xyz = act.contiguous(), xyz.contiguous()
    dev = act.device
    thr = _device_thresholds(sed_threshold, n_classes, dev)
    rows = torch.empty((n_files, 3 * n_frames * n_classes, 4), dtype=torch.int16, device=dev)
    counts = torch.empty((n_files,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        export = _lib.load().salsa_nn_seld_decode_multi if thr is None else _lib.load().salsa_nn_seld_decode_multi_thr
        rc = export(_ptr(act), _ptr(xyz), n_files, n_in, n_frames, n_classes, float(sed_threshold) if thr is None else _ptr(thr),
                    cos_unify, _ptr(rows), _ptr(counts), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == _lib.E_INVAL:
        raise ValueError('salsa_nn_seld_decode_multi refused %d files of %d frames (%d decoded) x %d classes' % (n_files, n_in, n_frames, n_classes))
    if rc:
        raise RuntimeError('salsa_nn_seld_decode_multi failed (%d)' % rc)
    return rows, counts


def chunk_merge_multi(act, xyz, chunk_len: int, chunk_hop: int, n_frames: int = 600, n_classes: int = 12):
    """The chunk combine of track_merge='align' on the device: Multi-ACCDOA chunk outputs act (n_files, n_chunks,
    chunk_len, 3 C) and xyz (.., 9 C), CUDA float32 at the label rate, chunk_len / chunk_hop in label frames -> file outputs
    (n_files, n_frames, 3 C) and (.., 9 C), decode_multi_rows' input: overlapping frames are averaged pairwise in chunk order after
    the fresh chunk's tracks are aligned, cell by cell, to the running value.  One salsa_nn_chunk_merge_multi launch on the current
    stream, no synchronisation; CPU tensors are refused (the host function is postprocess.combine_chunks_multi, whose result this
    equals bit for bit)."""
    import torch
    if act.dim() != 4 or xyz.dim() != 4 or act.shape[:3] != xyz.shape[:3] or act.shape[3] != 3 * n_classes or xyz.shape[3] != 9 * n_classes:
        raise ValueError('chunk_merge_multi: act %s / xyz %s are not (files, chunks, frames, %d) / (.., %d)'
                         % (tuple(act.shape), tuple(xyz.shape), 3 * n_classes, 9 * n_classes))
    if not (act.is_cuda and xyz.is_cuda and act.device == xyz.device and act.dtype == torch.float32 and xyz.dtype == torch.float32):
        raise ValueError('chunk_merge_multi takes float32 tensors on one CUDA device (the host path is postprocess.combine_chunks_multi)')
    n_files, n_chunks, L = act.shape[:3]
    if L != chunk_len:
        raise ValueError('chunk_merge_multi: chunks of %d frames, chunk_len = %d' % (L, chunk_len))
    if n_files == 0:
        raise ValueError('chunk_merge_multi: no files')
    act, xyz = act.contiguous(), xyz.contiguous()
    dev = act.device
    fa = torch.empty((n_files, n_frames, 3 * n_classes), dtype=torch.float32, device=dev)
    fx = torch.empty((n_files, n_frames, 9 * n_classes), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().salsa_nn_chunk_merge_multi(_ptr(act), _ptr(xyz), n_files, n_chunks, chunk_len, chunk_hop, n_frames, n_classes,
                                                    _ptr(fa), _ptr(fx), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc == _lib.E_INVAL:
        raise ValueError('salsa_nn_chunk_merge_multi refused: ' + _lib.last_error())
    if rc:
        raise RuntimeError('salsa_nn_chunk_merge_multi failed (%d)' % rc)
    return fa, fx


def rows_to_list(rows, counts, eval_version: str = '2021', as_array: bool = False) -> list:
    """decode_dcase_rows' rows (n_files, capacity, 4) and counts (n_files,) ON THE HOST (numpy arrays or CPU tensors) -> per file
    exactly what to_dcase_rows returns: [frame, class, 0, azimuth, elevation] rows for eval_version '2021' and '2022' (the zero track column
    is added here), [frame, class, azimuth, elevation] otherwise; int64, a list of lists or with as_array one (n, 5 | 4) array."""
    rows = rows.numpy() if hasattr(rows, 'numpy') else np.asarray(rows)
    counts = counts.numpy() if hasattr(counts, 'numpy') else np.asarray(counts)
    out = []
    for f in range(rows.shape[0]):
        r = rows[f, :int(counts[f])].astype(np.int64)
        if eval_version in ('2021', '2022'):
            r = np.concatenate([r[:, :2], np.zeros((r.shape[0], 1), dtype=np.int64), r[:, 2:]], axis=1)
        out.append(r if as_array else r.tolist())
    return out
