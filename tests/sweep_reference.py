"""Reference and inputs of the threshold-sweep tests (tests/test_threshold_sweep_cpu.py, tests/test_threshold_sweep_gpu.py).

`brute_force`: per candidate k and class c the file is decoded by the host decoder at the SCALAR threshold thresholds[k, c] (the
decoders' original, scalar code path), the rows of class c are kept, and the union over the classes is scored by
SeldMetrics2022.update -- float64, nothing shared between candidates.  `expected_status` says, from numpy's own distances, which
(segment, candidate, class) entries the device statements must hand to the host: 1 where another pairing of a common cell costs
within `margin` of the best or a slot average lies within `margin` of the DOA threshold, 2 where a reference cell of the class holds
more than 4 DOAs.

`planted_case` builds the small inputs both test files use: 3 files x 25 frames at label rate 10 (a 5-frame last segment), 3 classes,
6 candidates, with every edge the issue names planted at known places."""
import itertools

import numpy as np

GRID = np.array([0.05, 0.2, 0.3, 0.5, 0.7, 1.5], dtype=np.float32)         # below every activity ... above every activity
N_FILES, N_FRAMES, RATE, C = 3, 25, 10, 3
DOA_THRESHOLD = 20
RANDOM_SEED = 7                                                            # of the 2 x 600 x 12 random case (checked for doubts on the CPU)


def host_rows(act, xyz, thr, n_frames, n_classes, fmt, unify_deg):
    from salsa_amd.crnn.postprocess import multi_accdoa_rows, to_dcase_rows
    if fmt == 'multi_accdoa':
        return multi_accdoa_rows(act, xyz, sed_threshold=thr, unify_deg=unify_deg, n_classes=n_classes, max_nframes_per_file=n_frames,
                                 eval_version='2020')
    return to_dcase_rows(act, xyz, sed_threshold=thr, n_classes=n_classes, max_nframes_per_file=n_frames, eval_version='2020')


def rows_at(act, xyz, thr_vec, n_frames, n_classes, fmt, unify_deg):
    """the rows at a threshold VECTOR, through scalar decoder calls only: class c's rows from the call at thr_vec[c]"""
    rows = []
    for c in range(n_classes):
        if thr_vec[c] != thr_vec[c]:                                      # a NaN threshold: the class is inactive
            continue
        rows += [r for r in host_rows(act, xyz, float(thr_vec[c]), n_frames, n_classes, fmt, unify_deg) if r[1] == c]
    return sorted(rows, key=lambda r: (r[0], r[1]))                        # (stable: a cell's rows keep their group order)


def brute_force(act, xyz, gt, thresholds, n_frames, n_classes, fmt='reg_xyz', unify_deg=15.0, doa_threshold=DOA_THRESHOLD, label_rate=RATE):
    """-> counters (files, K, C, 8) int64 in SeldMetrics2022.CLASS_COUNTERS' order and total_DE (files, K, C) float64"""
    from salsa_amd.crnn.metrics import SeldMetrics2022
    K = thresholds.shape[0]
    counters, de = np.zeros((len(act), K, n_classes, 8), np.int64), np.zeros((len(act), K, n_classes))
    for f in range(len(act)):
        for k in range(K):
            m = SeldMetrics2022(n_classes, doa_threshold)
            m.update(rows_at(act[f], xyz[f], thresholds[k], n_frames, n_classes, fmt, unify_deg), gt[f], max_frames=n_frames, label_rate=label_rate)
            counters[f, k] = np.stack([getattr(m, n) for n in SeldMetrics2022.CLASS_COUNTERS], axis=1)
            de[f, k] = m.total_DE
    return counters, de


def _class_status(pred, gt, doa_threshold, margin):
    """one class of one segment (rows with the frame counted in the segment) -> 0 | 1 | 2, by numpy's distances"""
    from salsa_amd.crnn.metrics import angular_distance_deg
    g, p = {}, {}
    for r in gt:
        g.setdefault(r[0], []).append((r[2], r[3]))
    for r in pred:
        p.setdefault(r[0], []).append((r[2], r[3]))
    if g and max(len(v) for v in g.values()) > 4:
        return 2
    if not g or not p:
        return 0
    doubt, per_slot = False, {}
    for frame, gd in g.items():
        if frame not in p:
            continue
        ga, pa = np.array(gd, np.float64), np.array(p[frame], np.float64)
        cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
        ng, n_p = cost.shape
        small, large = min(ng, n_p), max(ng, n_p)
        maps = []
        for perm in itertools.permutations(range(large), small):
            pairs = [(i, to) if ng <= n_p else (to, i) for i, to in enumerate(perm)]
            maps.append((sum(cost[r, q] for r, q in pairs), pairs))
        maps.sort(key=lambda m: m[0])
        if len(maps) > 1 and maps[1][0] - maps[0][0] <= margin:
            doubt = True
        for r, q in maps[0][1]:
            per_slot.setdefault(r, []).append(cost[r, q])
    for d in per_slot.values():
        if abs(sum(d) / len(d) - doa_threshold) <= margin:
            doubt = True
    return 1 if doubt else 0


def expected_status(act, xyz, gt, thresholds, n_frames, n_classes, fmt, unify_deg, margin, doa_threshold=DOA_THRESHOLD, label_rate=RATE):
    """-> (files, n_seg, K, C) int32"""
    n_seg = -(-n_frames // label_rate)
    out = np.zeros((len(act), n_seg, thresholds.shape[0], n_classes), np.int32)
    for f in range(len(act)):
        for k in range(thresholds.shape[0]):
            pred = rows_at(act[f], xyz[f], thresholds[k], n_frames, n_classes, fmt, unify_deg)
            for s in range(n_seg):
                seg = lambda rows: [(r[0] - s * label_rate,) + tuple(r[1:]) for r in rows if s * label_rate <= r[0] < (s + 1) * label_rate]
                ps, gs = seg(pred), seg(gt[f])
                for c in range(n_classes):
                    out[f, s, k, c] = _class_status([r for r in ps if r[1] == c], [r for r in gs if r[1] == c], doa_threshold, margin)
    return out


def angles_of(v):
    """integer (azimuth, elevation) of float32 vectors (.., 3), as csrc/seld_decode.h rounds them"""
    v = np.asarray(v, np.float32).astype(np.float64)
    azi = np.around(np.arctan2(v[..., 1], v[..., 0]) * 180.0 / np.pi).astype(np.int64)
    ele = np.around(np.arctan2(v[..., 2], np.sqrt(v[..., 0] ** 2 + v[..., 1] ** 2)) * 180.0 / np.pi).astype(np.int64)
    return np.where(azi == 180, -180, azi), ele


def unit(azi, ele):
    a, e = np.deg2rad(azi), np.deg2rad(ele)
    return np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], np.float32)


def random_case(seed, n_files, n_frames, n_classes, fmt, gt_density=0.4):
    """activities in [0.1, 0.95], random directions, references near the (first track's) predicted direction in a fraction of the
    cells -> act (files, T, nc | 3 C), xyz (files, T, 3 nc | 9 C) float32 and gt, per file a list of (frame, class, azimuth, elevation)"""
    rng = np.random.RandomState(seed)
    tracks = 3 if fmt == 'multi_accdoa' else 1
    act = rng.uniform(0.1, 0.95, (n_files, n_frames, tracks * n_classes)).astype(np.float32)
    v = rng.standard_normal((n_files, n_frames, 3, tracks, n_classes)).astype(np.float32)     # (axis, track, class): column (tracks a + n) C + c
    xyz = v.reshape(n_files, n_frames, 3 * tracks * n_classes)
    azi, ele = angles_of(np.moveaxis(v[:, :, :, 0, :], 2, -1))                               # track 0's direction per (file, frame, class)
    gt = []
    for f in range(n_files):
        rows = []
        for t, c in zip(*np.nonzero(rng.uniform(size=(n_frames, n_classes)) < gt_density)):
            a = (int(azi[f, t, c]) + int(rng.randint(-30, 31)) + 180) % 360 - 180
            e = int(np.clip(int(ele[f, t, c]) + int(rng.randint(-10, 11)), -90, 90))
            rows.append((int(t), int(c), a, e))
        gt.append(rows)
    return act, xyz, gt


def planted_case(fmt):
    """-> dict(act, xyz, gt, thresholds (6, 3), fmt, unify_deg, planted): the random case of 3 x 25 x 3 with, on top of it,
      file 0, frame 3, class 1   an activity exactly float32(0.3), a candidate's value (active at it, by >=)
      file 0, frame 4, class 2   a NaN activity with a NaN direction (never active); multi: also a NaN direction on an active track
      file 0, frame 6, class 0   two references of the class in one frame
      file 1, segment 0, class 2 one reference, in frame 2, exactly 20 degrees from the prediction (1, 0, 0): the slot average is the
                                 threshold wherever frame 2 is active -- doubt at those candidates
      file 1, frame 12, class 0  five references in one cell: class 0 of segment 1 is refused at every candidate
      multi, file 2, frame 1, class 1   tracks 0 and 1 five degrees apart with activities 0.6 and 0.4: unified at 0.3, alone at 0.5
    every class column of `thresholds` is GRID, class 2's shifted by one place, so the candidates are a (K, C) table"""
    multi = fmt == 'multi_accdoa'
    tracks = 3 if multi else 1
    act, xyz, gt = random_case(11, N_FILES, N_FRAMES, C, fmt)
    col = lambda a, n, c: (tracks * a + n) * C + c
    act[0, 3, 1] = np.float32(0.3)
    for n in range(tracks):
        act[0, 4, n * C + 2] = np.nan
    for a in range(3):
        xyz[0, 4, col(a, 0, 2)] = np.nan
    if multi:
        act[0, 5, 0 * C + 2] = 0.9
        xyz[0, 5, col(1, 0, 2)] = np.nan
    gt[0] = [r for r in gt[0] if (r[0], r[1]) != (6, 0)] + [(6, 0, 10, 5), (6, 0, -120, 30)]
    # the 20-degree slot: class 2 of file 1 has one reference in segment 0, against the prediction (1, 0, 0) of every track
    gt[1] = [r for r in gt[1] if not (r[0] < RATE and r[1] == 2)] + [(2, 2, 20, 0)]
    for n in range(tracks):
        act[1, 2, n * C + 2] = 0.6 if n == 0 else 0.01                                       # (other tracks: never active, below every candidate)
        for a in range(3):
            xyz[1, 2, col(a, n, 2)] = 1.0 if a == 0 else 0.0
    gt[1] = [r for r in gt[1] if (r[0], r[1]) != (12, 0)] + [(12, 0, 10 * i, 5 * i) for i in range(5)]
    if multi:
        act[2, 1, 0 * C + 1], act[2, 1, 1 * C + 1], act[2, 1, 2 * C + 1] = 0.6, 0.4, 0.01
        for a in range(3):
            xyz[2, 1, col(a, 0, 1)], xyz[2, 1, col(a, 1, 1)] = unit(40, 10)[a], unit(45, 10)[a]
        gt[2] = [r for r in gt[2] if (r[0], r[1]) != (1, 1)] + [(1, 1, 42, 10)]
    thresholds = np.repeat(GRID[:, None], C, axis=1)
    thresholds[:, 2] = np.roll(GRID, 1)
    return dict(act=act, xyz=xyz, gt=gt, thresholds=thresholds, fmt=fmt, unify_deg=15.0)
