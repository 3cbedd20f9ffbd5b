"""SELD evaluation of DCASE-format outputs: location-sensitive detection (ER, F) and class-sensitive localisation (LE, LR)
over 1-s segments, as the reference computes them (metrics/SELD2021_evaluation_metrics.py:81-195 SELDMetrics,
metrics/dcase_utils.py:8-57 load_output_format_file, :185-228 segment_labels; driven by models/interfaces.py:163-180).
Host bookkeeping on a few thousand CSV rows per clip: numpy + scipy's Hungarian solver, no device work.

A "row" is (frame, class, azimuth_deg, elevation_deg[, track]).  Within one segment and class, every frame holds a list
of DOAs; reference and predicted DOAs of a common frame are paired by minimum total great-circle distance, distances
are averaged per reference slot (its position in the frame's list -- the reference ignores track ids), and a slot counts
as a true positive when its average is within ``doa_threshold`` degrees."""
import csv

import numpy as np
from scipy.optimize import linear_sum_assignment

_EPS = np.finfo(float).eps


def load_dcase_csv(path: str, version: str = '2021'):
    """DCASE output-format CSV -> list of (frame, class, azimuth, elevation, track).  4 columns: submission rows
    (frame, class, azi, ele); 5 columns: (frame, class, track, azi, ele).  (dcase_utils.py:8-57, polar formats.)  The 2022 row
    format is the 2021 one."""
    if version not in ('2020', '2021', '2022'):
        raise ValueError('version {} is not implemented'.format(version))
    rows = []
    with open(path, 'r', newline='') as f:
        for w in csv.reader(f):
            if not w:
                continue
            if len(w) == 4:
                rows.append((int(w[0]), int(w[1]), float(w[2]), float(w[3]), 0))
            elif len(w) == 5:
                rows.append((int(w[0]), int(w[1]), float(w[3]), float(w[4]), int(w[2])))
            else:
                raise ValueError('Cartesian (6-column) rows are not used on this path')
    return rows


def segment_rows(rows, max_frames: int = 600, label_rate: int = 10):
    """rows -> {segment: {class: {frame_in_segment: [(azi, ele), ...]}}} in arrival order (dcase_utils.py:185-228)."""
    n_seg = int(np.ceil(max_frames / float(label_rate)))
    seg = {s: {} for s in range(n_seg)}
    for frame, cls, azi, ele, *_ in rows:
        if 0 <= frame < n_seg * label_rate:
            seg[frame // label_rate].setdefault(cls, {}).setdefault(frame % label_rate, []).append((azi, ele))
    return seg


def angular_distance_deg(azi1, ele1, azi2, ele2):
    """Great-circle distance in degrees between polar directions given in degrees (SELD2021...:198-209)."""
    a1, e1, a2, e2 = (np.asarray(v, dtype=np.float64) * np.pi / 180. for v in (azi1, ele1, azi2, ele2))
    d = np.sin(e1) * np.sin(e2) + np.cos(e1) * np.cos(e2) * np.cos(np.abs(a1 - a2))
    return np.arccos(np.clip(d, -1, 1)) * 180 / np.pi


class SeldMetrics:
    def __init__(self, n_classes: int = 12, doa_threshold: float = 20):
        self.n_classes, self.doa_threshold = n_classes, doa_threshold
        self.TP = self.FP = self.FN = 0
        self.S = self.D = self.I = self.Nref = 0
        self.total_DE = 0.0
        self.DE_TP = self.DE_FP = self.DE_FN = 0

    def update(self, pred_rows, gt_rows, max_frames: int = 600, label_rate: int = 10):
        pred, gt = segment_rows(pred_rows, max_frames, label_rate), segment_rows(gt_rows, max_frames, label_rate)
        for s in range(len(gt)):
            seg_fn = seg_fp = 0
            for c in range(self.n_classes):
                g, p = gt[s].get(c), pred[s].get(c)
                n_g = max(len(v) for v in g.values()) if g else 0
                n_p = max(len(v) for v in p.values()) if p else 0
                self.Nref += n_g
                if g and p:
                    per_slot = {}                                          # reference slot -> distances of its pairings
                    for frame, g_doas in g.items():
                        if frame not in p:
                            continue
                        ga, pa = np.array(g_doas, dtype=np.float64), np.array(p[frame], dtype=np.float64)
                        cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
                        ri, ci = linear_sum_assignment(cost)
                        for r, col in zip(ri, ci):
                            per_slot.setdefault(int(r), []).append(cost[r, col])
                    if not per_slot:         # no frame in common: the reference books the PREDICTED count as misses (:141-146)
                        seg_fn += n_p
                        self.FN += n_p
                        self.DE_FN += n_p
                    else:
                        for dists in per_slot.values():
                            avg = sum(dists) / len(dists)
                            self.total_DE += avg
                            self.DE_TP += 1
                            if avg <= self.doa_threshold:
                                self.TP += 1
                            else:
                                seg_fp += 1
                                self.FP += 1
                        if n_p > n_g:
                            seg_fp += n_p - n_g
                            self.FP += n_p - n_g
                            self.DE_FP += n_p - n_g
                        elif n_p < n_g:
                            seg_fn += n_g - n_p
                            self.FN += n_g - n_p
                            self.DE_FN += n_g - n_p
                elif g:
                    seg_fn += n_g
                    self.FN += n_g
                    self.DE_FN += n_g
                elif p:
                    seg_fp += n_p
                    self.FP += n_p
                    self.DE_FP += n_p
            self.S += min(seg_fp, seg_fn)
            self.D += max(0, seg_fn - seg_fp)
            self.I += max(0, seg_fp - seg_fn)

    def scores(self):
        """-> (ER, F, LE, LR) (SELD2021...:56-78)."""
        ER = (self.S + self.D + self.I) / float(self.Nref + _EPS)
        F = self.TP / (_EPS + self.TP + 0.5 * (self.FP + self.FN))
        LE = self.total_DE / float(self.DE_TP + _EPS) if self.DE_TP else 180
        LR = self.DE_TP / (_EPS + self.DE_TP + self.DE_FN)
        return ER, F, LE, LR

    def seld_error(self):
        """Aggregate used for model selection (interfaces.py:179): mean of ER, 1-F, LE/180, 1-LR."""
        ER, F, LE, LR = self.scores()
        return (ER + (1.0 - F) + LE / 180.0 + (1.0 - LR)) / 4


class SeldMetrics2020:
    """The SELD 2020 metric (metrics/SELD2020_evaluation_metrics.py:159-229 update_seld_scores, :49-83 compute_seld_scores, :266-294
    least_distance_between_gt_pred), the scorer the reference's eval_version '2020' selects (models/interfaces.py:46-53).  Per 1-s
    segment and class it counts PRESENCE (Nref, Nsys), not tracks; where both sides hold the class, the reference frames are walked
    in ascending frame order (dcase_utils.segment_labels walks the audio frames in order, whatever the order of the rows), every
    frame that also has predictions costs the minimum total distance of pairing the smaller side into the larger -- only the value
    of that minimum enters, not the pairing -- and the class is a hit when the mean cost over those frames is within
    ``doa_threshold`` degrees; a miss of any kind is a false NEGATIVE.  Same surface as SeldMetrics."""

    def __init__(self, n_classes: int = 12, doa_threshold: float = 20):
        self.n_classes, self.doa_threshold = n_classes, doa_threshold
        self.TP = self.FP = self.FN = self.TN = 0
        self.S = self.D = self.I = 0
        self.Nref = self.Nsys = 0
        self.total_DE = 0.0
        self.DE_TP = 0

    def update(self, pred_rows, gt_rows, max_frames: int = 600, label_rate: int = 10):
        pred, gt = segment_rows(pred_rows, max_frames, label_rate), segment_rows(gt_rows, max_frames, label_rate)
        for s in range(len(gt)):
            loc_fn = loc_fp = 0
            for c in range(self.n_classes):
                g, p = gt[s].get(c), pred[s].get(c)
                self.Nref += 1 if g else 0
                self.Nsys += 1 if p else 0
                if g and p:
                    total, n = 0.0, 0
                    for frame in sorted(g):                                # ascending frames; DOAs inside a frame keep file order
                        if frame not in p:
                            continue
                        ga, pa = np.array(g[frame], dtype=np.float64), np.array(p[frame], dtype=np.float64)
                        cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
                        if cost.shape == (1, 1):
                            total += cost[0, 0]
                        else:
                            ri, ci = linear_sum_assignment(cost)
                            total += cost[ri, ci].sum()                    # (at most 4 values: numpy adds them in reference-row order)
                        n += 1
                    if n == 0:                                             # no frame in common
                        loc_fn += 1
                        self.FN += 1
                    else:
                        avg = total / n
                        self.total_DE += avg
                        self.DE_TP += 1
                        if avg <= self.doa_threshold:
                            self.TP += 1
                        else:
                            loc_fn += 1
                            self.FN += 1
                elif g:
                    loc_fn += 1
                    self.FN += 1
                elif p:
                    loc_fp += 1
                    self.FP += 1
                else:
                    self.TN += 1
            self.S += min(loc_fp, loc_fn)
            self.D += max(0, loc_fn - loc_fp)
            self.I += max(0, loc_fp - loc_fn)

    def scores(self):
        """-> (ER, F, LE, LR) (SELD2020...:49-83, eps where the reference places it).  The reference itself raises ZeroDivisionError
        on an empty reference, in an auxiliary list it never returns (Nsys / Nref); that list is not computed here."""
        ER = (self.S + self.D + self.I) / float(self.Nref + _EPS)
        prec, recall = float(self.TP) / float(self.Nsys + _EPS), float(self.TP) / float(self.Nref + _EPS)
        F = 2 * prec * recall / (prec + recall + _EPS)
        LE = self.total_DE / float(self.DE_TP + _EPS) if self.DE_TP else 180
        de_prec, de_recall = float(self.DE_TP) / float(self.Nsys + _EPS), float(self.DE_TP) / float(self.Nref + _EPS)
        LR = 2 * de_prec * de_recall / (de_prec + de_recall + _EPS)
        return ER, F, LE, LR

    def seld_error(self):
        """Aggregate used for model selection (interfaces.py:179): mean of ER, 1-F, LE/180, 1-LR."""
        ER, F, LE, LR = self.scores()
        return (ER + (1.0 - F) + LE / 180.0 + (1.0 - LR)) / 4


class SeldMetrics2022:
    """The class-wise SELD metric of DCASE 2022 and later: this project's own restatement of the public DCASE 2022 metric (the
    upstream repository has no 2022 metric file), the figure reported for Multi-ACCDOA systems.  `update`
    makes the walk of SeldMetrics.update, statement for statement -- segments, classes in order, reference frames in arrival order,
    linear_sum_assignment on angular_distance_deg, distances averaged per reference slot, the "no common frame" rule -- and only
    where the bookkeeping lands changes: the counters TP FP FP_spatial FN Nref DE_TP DE_FP DE_FN are int64 arrays over the classes
    and total_DE a float64 one (S, D, I stay scalars, formed per segment over all classes), and a slot average above the threshold
    adds to FP_spatial[c] (and to the segment's false positives behind S, D, I), not to FP[c].  Per class therefore FP == DE_FP,
    FN == DE_FN and FP_spatial == DE_TP - TP.

    average='macro' (the published figure): F, LE, LR and seld_error() are plain means over ALL n_classes classes, with the DCASE
    2022 semantics that a class absent from both sides counts with F 0, LE 180 and LR 0 -- choose n_classes to match the data.
    average='micro': the same expressions on the class sums.  ER is (S + D + I) / Nref over all classes either way.

    Every `update` call is one file and its counters are kept per file as well (`file_records`), which is what `jackknife` leaves
    out one at a time."""

    CLASS_COUNTERS = ('TP', 'FP', 'FP_spatial', 'FN', 'Nref', 'DE_TP', 'DE_FP', 'DE_FN')

    def __init__(self, n_classes: int = 12, doa_threshold: float = 20, average: str = 'macro'):
        if average not in ('macro', 'micro'):
            raise ValueError('average must be macro or micro, not {!r}'.format(average))
        self.n_classes, self.doa_threshold, self.average = n_classes, doa_threshold, average
        for name in self.CLASS_COUNTERS:
            setattr(self, name, np.zeros(n_classes, dtype=np.int64))
        self.total_DE = np.zeros(n_classes, dtype=np.float64)
        self.S = self.D = self.I = 0
        self._files = []                                                   # per file: (class counters (C, 8), total_DE (C,), S D I (3,))

    def _add(self, cls, de, sdi, file=None):
        """counters of a whole file (file=None: a new file record) or of a part of file `file` into the totals and the file's record"""
        for k, name in enumerate(self.CLASS_COUNTERS):
            setattr(self, name, getattr(self, name) + cls[:, k])
        self.total_DE = self.total_DE + de
        self.S, self.D, self.I = self.S + int(sdi[0]), self.D + int(sdi[1]), self.I + int(sdi[2])
        if file is None:
            self._files.append((cls.copy(), de.copy(), sdi.copy()))
        else:
            old = self._files[file]
            self._files[file] = (old[0] + cls, old[1] + de, old[2] + sdi)

    def _add_files(self, cls, de, sdi):
        """_add for many new files at once: class counters (n, C, 8), total_DE (n, C), S D I (n, 3), added in file order"""
        for k, name in enumerate(self.CLASS_COUNTERS):
            setattr(self, name, getattr(self, name) + cls[:, :, k].sum(axis=0))
        self.total_DE = self.total_DE + np.add.reduce(de, axis=0)
        self.S, self.D, self.I = (int(v) for v in np.array([self.S, self.D, self.I]) + sdi.sum(axis=0))
        self._files += list(zip(cls, de, sdi))

    def update(self, pred_rows, gt_rows, max_frames: int = 600, label_rate: int = 10):
        pred, gt = segment_rows(pred_rows, max_frames, label_rate), segment_rows(gt_rows, max_frames, label_rate)
        TP, FP, FP_spatial, FN, Nref, DE_TP, DE_FP, DE_FN = cls = np.zeros((8, self.n_classes), dtype=np.int64)
        total_DE, sdi = np.zeros(self.n_classes, dtype=np.float64), np.zeros(3, dtype=np.int64)
        for s in range(len(gt)):
            seg_fn = seg_fp = 0
            for c in range(self.n_classes):
                g, p = gt[s].get(c), pred[s].get(c)
                n_g = max(len(v) for v in g.values()) if g else 0
                n_p = max(len(v) for v in p.values()) if p else 0
                Nref[c] += n_g
                if g and p:
                    per_slot = {}                                          # reference slot -> distances of its pairings
                    for frame, g_doas in g.items():
                        if frame not in p:
                            continue
                        ga, pa = np.array(g_doas, dtype=np.float64), np.array(p[frame], dtype=np.float64)
                        cost = angular_distance_deg(ga[:, None, 0], ga[:, None, 1], pa[None, :, 0], pa[None, :, 1])
                        ri, ci = linear_sum_assignment(cost)
                        for r, col in zip(ri, ci):
                            per_slot.setdefault(int(r), []).append(cost[r, col])
                    if not per_slot:         # no frame in common: the PREDICTED count is booked as misses, as SeldMetrics does
                        seg_fn += n_p
                        FN[c] += n_p
                        DE_FN[c] += n_p
                    else:
                        for dists in per_slot.values():
                            avg = sum(dists) / len(dists)
                            total_DE[c] += avg
                            DE_TP[c] += 1
                            if avg <= self.doa_threshold:
                                TP[c] += 1
                            else:                                          # right class, wrong place: a false positive of its own kind
                                seg_fp += 1
                                FP_spatial[c] += 1
                        if n_p > n_g:
                            seg_fp += n_p - n_g
                            FP[c] += n_p - n_g
                            DE_FP[c] += n_p - n_g
                        elif n_p < n_g:
                            seg_fn += n_g - n_p
                            FN[c] += n_g - n_p
                            DE_FN[c] += n_g - n_p
                elif g:
                    seg_fn += n_g
                    FN[c] += n_g
                    DE_FN[c] += n_g
                elif p:
                    seg_fp += n_p
                    FP[c] += n_p
                    DE_FP[c] += n_p
            sdi[0] += min(seg_fp, seg_fn)
            sdi[1] += max(0, seg_fn - seg_fp)
            sdi[2] += max(0, seg_fp - seg_fn)
        self._add(cls.T, total_DE, sdi)

    def merge(self, other):
        """adds another scorer's counters and appends its file records"""
        if (other.n_classes, other.doa_threshold) != (self.n_classes, self.doa_threshold):
            raise ValueError('merge: scores of %d classes at %s degrees into %d classes at %s degrees'
                             % (other.n_classes, other.doa_threshold, self.n_classes, self.doa_threshold))
        for rec in list(other._files):
            self._add(*rec)
        return self

    def file_records(self):
        """-> dict: every class counter and total_DE as (n_files, n_classes) arrays, S, D, I as (n_files,) arrays, in update order"""
        C = self.n_classes
        cls = np.stack([f[0] for f in self._files]) if self._files else np.zeros((0, C, len(self.CLASS_COUNTERS)), dtype=np.int64)
        out = {name: cls[:, :, k] for k, name in enumerate(self.CLASS_COUNTERS)}
        out['total_DE'] = np.stack([f[1] for f in self._files]) if self._files else np.zeros((0, C))
        sdi = np.stack([f[2] for f in self._files]) if self._files else np.zeros((0, 3), dtype=np.int64)
        out.update(S=sdi[:, 0], D=sdi[:, 1], I=sdi[:, 2])
        return out

    def _totals(self):
        return np.stack([getattr(self, n) for n in self.CLASS_COUNTERS], axis=1), self.total_DE, np.array([self.S, self.D, self.I], dtype=np.int64)

    @staticmethod
    def _classwise(cls, de, sdi):
        """class counters (C, 8), total_DE (C,), S D I -> (C, 5) ER F_c LE_c LR_c SELD_c"""
        TP, FP, FP_spatial, FN, Nref, DE_TP, _, DE_FN = (cls[:, k].astype(np.float64) for k in range(8))
        ER = float(sdi.sum()) / float(cls[:, 4].sum() + _EPS)
        F = TP / (_EPS + TP + FP_spatial + 0.5 * (FP + FN))
        LE = np.where(DE_TP > 0, de / (DE_TP + _EPS), 180.0)
        LR = DE_TP / (_EPS + DE_TP + DE_FN)
        return np.stack([np.full_like(F, ER), F, LE, LR, (ER + (1.0 - F) + LE / 180.0 + (1.0 - LR)) / 4], axis=1)

    def _scores_of(self, cls, de, sdi):
        """-> (ER, F, LE, LR, SELD) of the given counters by self.average"""
        if self.average == 'macro':
            return tuple(float(v) for v in self._classwise(cls, de, sdi).mean(axis=0))
        ER = float(sdi.sum()) / float(cls[:, 4].sum() + _EPS)
        TP, FP, FP_spatial, FN, _, DE_TP, _, DE_FN = (int(v) for v in cls.sum(axis=0))
        F = TP / (_EPS + TP + FP_spatial + 0.5 * (FP + FN))
        LE = float(de.sum()) / float(DE_TP + _EPS) if DE_TP else 180
        LR = DE_TP / (_EPS + DE_TP + DE_FN)
        return ER, F, LE, LR, (ER + (1.0 - F) + LE / 180.0 + (1.0 - LR)) / 4

    def classwise(self):
        """-> (n_classes, 5) array of ER (the same for every class), F_c, LE_c (180 where DE_TP[c] == 0), LR_c and
        SELD_c = mean(ER, 1 - F_c, LE_c / 180, 1 - LR_c)"""
        return self._classwise(*self._totals())

    def scores(self):
        """-> (ER, F, LE, LR), _EPS where SeldMetrics.scores places it.  macro: F, LE, LR are the means of classwise() over all
        n_classes classes; micro: the expressions on the class sums, F = TP / (eps + TP + FP_spatial + 0.5 (FP + FN))."""
        return self._scores_of(*self._totals())[:4]

    def seld_error(self):
        """Aggregate used for model selection.  macro: the mean of SELD_c over all classes; micro: mean of ER, 1-F, LE/180, 1-LR."""
        return self._scores_of(*self._totals())[4]

    def jackknife(self, confidence: float = 0.95):
        """Leave-one-file-out jackknife of ER, F, LE, LR and SELD (by self.average): with t the value from all n files and t_i the
        value from the totals minus file i, bias = (n - 1) (mean t_i - t), estimate = t - bias, std_err = sqrt((n - 1) / n
        sum (t_i - mean t_i)^2) and the interval estimate -+ t-quantile(1 - (1 - confidence) / 2, n - 1) std_err.
        -> {name: (estimate, bias, std_err, (lo, hi))}; ValueError for fewer than 2 files."""
        from scipy import stats
        n = len(self._files)
        if n < 2:
            raise ValueError('jackknife needs at least 2 files, not %d' % n)
        cls, de, sdi = self._totals()
        full = np.array(self._scores_of(cls, de, sdi))
        part = np.array([self._scores_of(cls - f[0], de - f[1], sdi - f[2]) for f in self._files])
        mean = part.mean(axis=0)
        bias = (n - 1) * (mean - full)
        estimate = full - bias
        std_err = np.sqrt((n - 1) / n * ((part - mean) ** 2).sum(axis=0))
        q = float(stats.t.ppf(1.0 - (1.0 - confidence) / 2.0, n - 1))
        return {name: (float(estimate[k]), float(bias[k]), float(std_err[k]), (float(estimate[k] - q * std_err[k]), float(estimate[k] + q * std_err[k])))
                for k, name in enumerate(('ER', 'F', 'LE', 'LR', 'SELD'))}


def evaluate_csv_dirs(pred_dir: str, gt_dir: str, filenames, n_classes: int = 12, doa_threshold: float = 20,
                      max_frames: int = 600, label_rate: int = 10, eval_version: str = '2021', average: str = 'macro'):
    """evaluate_output_prediction_csv (interfaces.py:163-180): -> (ER, F, LE, LR, seld_error) over the listed CSV files, by the
    metric class eval_version selects (interfaces.py:46-53): '2021' SeldMetrics, '2020' SeldMetrics2020; '2022' (this project's):
    SeldMetrics2022 with the given `average`, which the other two do not read."""
    import os
    if eval_version not in ('2020', '2021', '2022'):
        raise ValueError('Unknown eval_version {}'.format(eval_version))
    if eval_version == '2022':
        m = SeldMetrics2022(n_classes, doa_threshold, average)
    else:
        m = (SeldMetrics2020 if eval_version == '2020' else SeldMetrics)(n_classes, doa_threshold)
    for fn in filenames:
        m.update(load_dcase_csv(os.path.join(pred_dir, fn), version=eval_version),
                 load_dcase_csv(os.path.join(gt_dir, fn), version=eval_version), max_frames, label_rate)
    return m.scores() + (m.seld_error(),)
