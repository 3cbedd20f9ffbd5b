"""Inference post-processing of the SELD CRNN to the DCASE submission format (models/interfaces.py:97-139 combine_chunks,
:210-258 write_classwise_output_to_file): overlapping-chunk averaging, SED threshold, xyz -> azimuth/elevation in
integer degrees, one CSV row per (frame, active class).  CPU / numpy: it is bookkeeping on (600, 12) arrays."""
import csv

import numpy as np


def combine_chunks(frame_output_pred: np.ndarray, chunk_len: int, chunk_hop_len: int, n_frames: int = 600,
                   combine_method: str = 'mean') -> np.ndarray:
    """(n_chunks, chunk_len, C) label-rate chunk outputs -> (n_frames, C) file output; overlaps are averaged pairwise
    in arrival order exactly like the reference (a running (a+b)/2, not a uniform mean)."""
    out = np.zeros((n_frames,) + frame_output_pred.shape[2:], dtype=np.float32)
    starts = np.arange(0, n_frames - chunk_len + 1, chunk_hop_len).tolist()
    if (n_frames - chunk_len) % chunk_hop_len != 0:
        starts.append(n_frames - chunk_len)
    overlap = chunk_len - chunk_hop_len
    assert abs(frame_output_pred.shape[0] - len(starts)) < 2
    for i, s in enumerate(starts):
        e = s + chunk_len
        if i == 0:
            out[s:e] = frame_output_pred[i]
            continue
        if combine_method == 'mean':
            out[s:s + overlap] = (out[s:s + overlap] + frame_output_pred[i, :overlap]) / 2
        elif combine_method == 'gmean':
            out[s:s + overlap] = np.sqrt(out[s:s + overlap] * frame_output_pred[i, :overlap])
        else:
            raise ValueError('combine method {} is unknown'.format(combine_method))
        out[s + overlap:e] = frame_output_pred[i, overlap:]
    return out


def sed_from_accdoa(doa: np.ndarray, n_classes: int = 12) -> np.ndarray:
    """(..., 3 n_classes) ACCDOA xyz output -> (..., n_classes) SED activity: the length of each class's vector, in the input's
    precision (models/interfaces.py:260-268, get_sed_from_accdoa_output; float32 on the reference's inference path).  It is
    applied to the label-rate output of each chunk, before combine_chunks, as the reference does."""
    x = doa[..., :n_classes]
    y = doa[..., n_classes:2 * n_classes]
    z = doa[..., 2 * n_classes:]
    return np.sqrt(x ** 2 + y ** 2 + z ** 2)


def class_thresholds(sed_threshold, n_classes: int):
    """sed_threshold as every decoder compares it, in float32: a scalar -> np.float32; a sequence of n_classes values (one per class;
    for 'multi_accdoa' per REAL class, applied to its three tracks) -> a (n_classes,) float32 array.  A sequence of any other length
    is a ValueError -- raised here, before any device call.  A NaN threshold makes its class inactive (no activity is >= NaN)."""
    if np.ndim(sed_threshold) == 0:
        return np.float32(sed_threshold)
    thr = np.asarray(sed_threshold, dtype=np.float32)
    if thr.shape != (n_classes,):
        raise ValueError('sed_threshold: %s values for %d classes (a scalar, or one value per class)' % (thr.shape, n_classes))
    return thr


def to_dcase_rows(event_prob: np.ndarray, doa_xyz: np.ndarray, sed_threshold: float = 0.3, n_classes: int = 12,
                  max_nframes_per_file: int = 600, eval_version: str = '2021', as_array: bool = False):
    """event_prob (T, 12) sigmoid outputs, doa_xyz (T, 36) -> list of [frame, class, (0,) azimuth, elevation] rows, in the
    reference's order (frame ascending, class ascending within a frame: models/interfaces.py:232-258).  The reference walks the
    600 frames in a Python loop; here the active (frame, class) pairs come from one np.nonzero (row-major = the same order) and
    the angles are computed for those pairs only -- 1024 clips per inference step make the loop the bottleneck otherwise.
    as_array: the rows as one (n, 5 | 4) int64 array instead of a list of lists (bulk inference keeps them that way).
    sed_threshold: a scalar, or one value per class (class_thresholds: compared in float32, class c against its own value)."""
    if np.ndim(sed_threshold) == 0:
        active = event_prob >= sed_threshold
    else:
        active = event_prob[:, :n_classes] >= class_thresholds(sed_threshold, n_classes)
    assert active.shape[0] >= max_nframes_per_file, 'n_output_frames of sed < max_nframes_per_file'
    t, c = np.nonzero(active[:max_nframes_per_file, :n_classes])
    x, y, z = doa_xyz[t, c], doa_xyz[t, n_classes + c], doa_xyz[t, 2 * n_classes + c]
    azi = np.around(np.arctan2(y, x) * 180.0 / np.pi).astype(np.int64)
    ele = np.around(np.arctan2(z, np.sqrt(x ** 2 + y ** 2)) * 180.0 / np.pi).astype(np.int64)
    azi[azi == 180] = -180
    cols = [t, c, np.zeros_like(t), azi, ele] if eval_version in ('2021', '2022') else [t, c, azi, ele]
    rows = np.stack(cols, axis=1).astype(np.int64)
    return rows if as_array else rows.tolist()


def cos_unify_of(unify_deg: float) -> float:
    """the unification threshold of Multi-ACCDOA as the cosine every decision uses, computed once, in float64 on the host"""
    import math
    c = math.cos(float(unify_deg) * math.pi / 180.0)
    if not -1.0 <= c <= 1.0:
        raise ValueError('unify_deg %r has no cosine in [-1, 1]' % (unify_deg,))
    return c


def multi_accdoa_cells(act: np.ndarray, xyz: np.ndarray, sed_threshold: float, cos_unify: float, n_classes: int):
    """The per-cell rule of salsa_nn_seld_decode_multi (csrc/multi_accdoa.h, unify_cell) in numpy, statement for statement: act
    (T, 3 C), xyz (T, 9 C) float32 -> n_out (T, C) in 0 .. 3, out (T, C, 3, 3) float32 = the emitted vectors in group order (the
    groups behind n_out are zero) and flags (T, C): bit 0 sim01, bit 1 sim12, bit 2 sim20, bits 4 .. 6 the tracks' activity."""
    C = n_classes
    act, xyz = np.asarray(act, np.float32), np.asarray(xyz, np.float32)
    T = act.shape[0]
    assert act.shape == (T, 3 * C) and xyz.shape == (T, 9 * C), 'act (T, 3 C) / xyz (T, 9 C)'
    a = (act.reshape(T, 3, C) >= class_thresholds(sed_threshold, C)).transpose(0, 2, 1)   # (T, C, track); NaN is inactive; a (C,) vector: per class
    v = xyz.reshape(T, 3, 3, C).transpose(0, 3, 2, 1)                                  # (T, C, track, axis)
    d = v.astype(np.float64)

    def similar(i, j):
        xi, yi, zi, xj, yj, zj = d[..., i, 0], d[..., i, 1], d[..., i, 2], d[..., j, 0], d[..., j, 1], d[..., j, 2]
        dot = (xi * xj + yi * yj) + zi * zj
        ni, nj = (xi * xi + yi * yi) + zi * zi, (xj * xj + yj * yj) + zj * zj
        return a[..., i] & a[..., j] & (dot > cos_unify * np.sqrt(ni * nj))

    with np.errstate(invalid='ignore', over='ignore'):
        s01, s12, s20 = similar(0, 1), similar(1, 2), similar(2, 0)
        pair01, pair12, pair02 = ((v[..., 0, :] + v[..., 1, :]) / np.float32(2.0), (v[..., 1, :] + v[..., 2, :]) / np.float32(2.0),
                                  (v[..., 0, :] + v[..., 2, :]) / np.float32(2.0))
        triple = ((v[..., 0, :] + v[..., 1, :]) + v[..., 2, :]) / np.float32(3.0)
    flags = (s01.astype(np.int32) | s12.astype(np.int32) << 1 | s20.astype(np.int32) << 2
             | a[..., 0].astype(np.int32) << 4 | a[..., 1].astype(np.int32) << 5 | a[..., 2].astype(np.int32) << 6)
    n_sim = s01.astype(np.int32) + s12 + s20
    out = np.zeros((T, C, 3, 3), dtype=np.float32)
    n_out = np.zeros((T, C), dtype=np.int32)

    def emit(mask, vec):
        t, c = np.nonzero(mask)
        out[t, c, n_out[t, c]] = vec[t, c]
        n_out[t, c] += 1

    none, one = n_sim == 0, n_sim == 1
    for n in range(3):                                                                 # no similar pair: the active tracks, in order
        emit(none & a[..., n], v[..., n, :])
    emit(one & s01, pair01)                                                            # groups by their lowest track
    emit(one & s01 & a[..., 2], v[..., 2, :])
    emit(one & s12 & a[..., 0], v[..., 0, :])
    emit(one & s12, pair12)
    emit(one & s20, pair02)
    emit(one & s20 & a[..., 1], v[..., 1, :])
    emit(n_sim >= 2, triple)
    return n_out, out, flags


TRACK_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # csrc/multi_accdoa.h, source_of(3, cand, n)


def align_cells(anchor: np.ndarray, fresh: np.ndarray) -> np.ndarray:
    """csrc/track_align.h's align_cell in numpy, statement for statement: anchor, fresh (..., track, axis)
    float32 -> the candidate (..., ) int32 in 0 .. 5 whose permutation TRACK_PERMS[cand] of fresh's tracks is closest to anchor.  The
    cost is one running float64 sum, tracks outer and axes inner; a later candidate wins only when strictly smaller (explicit walk,
    not argmin: a NaN cost keeps candidate 0, a tie the lower index)."""
    R, V = np.asarray(anchor, np.float32).astype(np.float64), np.asarray(fresh, np.float32).astype(np.float64)
    chosen, best = np.zeros(R.shape[:-2], dtype=np.int32), None
    with np.errstate(invalid='ignore', over='ignore'):
        for cand, perm in enumerate(TRACK_PERMS):
            e = np.zeros(R.shape[:-2], dtype=np.float64)
            for n in range(3):
                for a in range(3):
                    d = R[..., n, a] - V[..., perm[n], a]
                    e = e + d * d
            if cand == 0:
                best = e
            else:
                less = e < best
                best, chosen = np.where(less, e, best), np.where(less, np.int32(cand), chosen)
    return chosen


def combine_chunks_multi(act: np.ndarray, xyz: np.ndarray, chunk_len: int, chunk_hop_len: int, n_frames: int = 600,
                         n_classes: int = 12):
    """combine_chunks for output_format 'multi_accdoa' under track_merge='align' (the host twin of
    salsa_nn_chunk_merge_multi and what decode='host' runs): one file's chunk outputs act (n_chunks, chunk_len, 3 C) and xyz
    (n_chunks, chunk_len, 9 C) at the label rate -> file outputs (n_frames, 3 C), (n_frames, 9 C) float32, multi_accdoa_rows' input.
    combine_chunks' walk per (frame, class) cell: chunk 0 is copied; of chunk i >= 1 the first chunk_len - chunk_hop_len frames are
    aligned to the running value (align_cells on the vectors) and become (old + new[pi]) / 2, activities with the same pi, and the
    rest overwrite.  One chunk at least as long as the file is placed and trimmed."""
    from .decode import chunk_starts
    C = n_classes
    act, xyz = np.asarray(act, np.float32), np.asarray(xyz, np.float32)
    n = act.shape[0]
    if act.shape != (n, chunk_len, 3 * C) or xyz.shape != (n, chunk_len, 9 * C):
        raise ValueError('combine_chunks_multi: act %s / xyz %s are not (chunks, %d, %d) / (.., %d)' % (act.shape, xyz.shape, chunk_len, 3 * C, 9 * C))
    starts = chunk_starts(n_frames, chunk_len, chunk_hop_len)
    if len(starts) != n or (n > 1 and chunk_hop_len > chunk_len):
        raise ValueError('combine_chunks_multi: %d chunks of %d frames at hop %d for %d frames (expected %d chunks)'
                         % (n, chunk_len, chunk_hop_len, n_frames, len(starts)))
    if n == 1:
        return act[0, :n_frames].copy(), xyz[0, :n_frames].copy()
    a = act.reshape(n, chunk_len, 3, C).transpose(0, 1, 3, 2)                          # (chunk, frame, class, track)
    v = xyz.reshape(n, chunk_len, 3, 3, C).transpose(0, 1, 4, 3, 2)                    # (chunk, frame, class, track, axis)
    out_a, out_v = np.zeros((n_frames, C, 3), np.float32), np.zeros((n_frames, C, 3, 3), np.float32)
    overlap, perms = chunk_len - chunk_hop_len, np.asarray(TRACK_PERMS)
    for i, s in enumerate(starts):
        if i == 0:
            out_a[s:s + chunk_len], out_v[s:s + chunk_len] = a[i], v[i]
            continue
        src = perms[align_cells(out_v[s:s + overlap], v[i, :overlap])]                 # (frame, class, track): the source of track n
        with np.errstate(invalid='ignore', over='ignore'):
            out_v[s:s + overlap] = (out_v[s:s + overlap] + np.take_along_axis(v[i, :overlap], src[..., None], axis=2)) / np.float32(2.0)
            out_a[s:s + overlap] = (out_a[s:s + overlap] + np.take_along_axis(a[i, :overlap], src, axis=2)) / np.float32(2.0)
        out_a[s + overlap:s + chunk_len], out_v[s + overlap:s + chunk_len] = a[i, overlap:], v[i, overlap:]
    return (np.ascontiguousarray(out_a.transpose(0, 2, 1)).reshape(n_frames, 3 * C),
            np.ascontiguousarray(out_v.transpose(0, 3, 2, 1)).reshape(n_frames, 9 * C))


def multi_accdoa_rows(act: np.ndarray, xyz: np.ndarray, sed_threshold: float = 0.5, unify_deg: float = 15.0, n_classes: int = 12,
                      max_nframes_per_file: int = 600, eval_version: str = '2021', as_array: bool = False):
    """The host decoder of output_format 'multi_accdoa' (what decode='host' runs and the yardstick of
    salsa_nn_seld_decode_multi): file-level track activities act (T, 3 n_classes) and vectors xyz (T, 9 n_classes) -> rows
    [frame, real class, (0,) azimuth, elevation] as to_dcase_rows shapes them, frame ascending, class ascending, then group order;
    tracks of one class closer than unify_deg degrees are unified (multi_accdoa_cells).  The angles are round-half-even of the
    float64 atan2 of the float32 vectors (csrc/seld_decode.h, xyz_to_angles; a NaN angle is written as 0)."""
    act, xyz = np.asarray(act, np.float32), np.asarray(xyz, np.float32)
    assert act.shape[0] >= max_nframes_per_file, 'n_output_frames < max_nframes_per_file'
    n_out, out, _ = multi_accdoa_cells(act[:max_nframes_per_file], xyz[:max_nframes_per_file], sed_threshold, cos_unify_of(unify_deg),
                                       n_classes)
    t, c, g = np.nonzero(np.arange(3)[None, None, :] < n_out[..., None])
    vec = out[t, c, g].astype(np.float64)
    x, y, z = vec[:, 0], vec[:, 1], vec[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        azi = np.around(np.arctan2(y, x) * 180.0 / np.pi)
        ele = np.around(np.arctan2(z, np.sqrt(x * x + y * y)) * 180.0 / np.pi)
    azi = np.where(np.isnan(azi), 0.0, azi).astype(np.int64)
    ele = np.where(np.isnan(ele), 0.0, ele).astype(np.int64)
    azi[azi == 180] = -180
    cols = [t, c, np.zeros_like(t), azi, ele] if eval_version in ('2021', '2022') else [t, c, azi, ele]
    rows = np.stack(cols, axis=1).astype(np.int64)
    return rows if as_array else rows.tolist()


def write_dcase_csv(path: str, rows) -> None:
    with open(path, 'w', newline='') as f:
        csv.writer(f).writerows(rows)
