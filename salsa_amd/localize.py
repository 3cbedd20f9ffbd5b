"""A model-free localiser on the features' directional channels.  The reference has no such code; the definition
is this project's.  Channels 4-6 of a SALSA (or SALSA-Lite) feature map hold one direction estimate per time-frequency bin.  For every
label frame (P feature frames) the bins of the columns [col0, col1) vote on an equal-angle grid over the sphere,

    score[g] = sum over the votes, in vote order, of max(0, (u . U[g] - c0) / (1 - c0)),      c0 = cos(kernel_deg),

a cap kernel that is linear in the cosine, and up to K peaks are picked greedily: the unsuppressed cell of greatest score (the lowest
index on a tie), stop below min_score, refine to the normalised sum of the votes within kernel_deg of the cell, suppress the cells within
suppress_deg of it.  A vote is u = (ch6, ch4, ch5) for FOA (the extractor writes Y, Z, X) and u = D^-1 (ch4, ch5, ch6) for MIC, D the
rows p_m - p_0 of the capsule positions (channel 3 + m is (p_m - p_0) . d in metres), normalised; a bin whose three values are zero (the
extractor's gate), not finite, or whose length lies outside norm_range casts none.  include/salsa_hip.h states the arithmetic to the
operation (salsa_doa_hist); the sums run in salsa_amd/csrc/doa_hist.hip, one launch for a whole batch.  SALSA_HIP_DOA=0 or a tensor on
the CPU goes to a composed torch evaluation of the same definition.

Two sources that overlap fully in time AND frequency are not separated: every bin then carries one blended direction."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .extractor import bin_limits
from .scenes import MIC_RADIUS, _unit

HIP_DOA = os.environ.get('SALSA_HIP_DOA', '1') != '0'      # 0: localize composes torch calls on the device too, for A/B runs and bisecting
MAX_VOTES, MAX_SOURCES = 4096, 8                            # the launcher's limits (include/salsa_hip.h: salsa_doa_hist_limits)
GRID_STEPS = (3, 5, 6, 9, 10, 15, 18, 30)                   # the divisors of 90 in 3 .. 30
MIC_FMAX_HZ = 1600.0                                        # below the rigid array's wrap at c / (2 x 1.5 x edge) = 1667 Hz
TORCH_ELEMENTS = 1 << 24                                    # (votes x cells) per step of the composed torch path


def doa_grid(step):
    """(azimuth, elevation) in integer degrees, int64 (G,), of the equal-angle grid: elevation -90 .. 90 in steps of `step`, each pole
    ONE cell (azimuth 0), elsewhere the azimuths -180 .. 180 - step; numbered elevation-major.  G = (360 / step)(180 / step - 1) + 2."""
    step = int(step)
    if step not in GRID_STEPS:
        raise ValueError('the grid step divides 90 and lies in 3 .. 30 degrees, got %r' % (step,))
    az, el = [0], [-90]
    for e in range(-90 + step, 90, step):
        a = np.arange(-180, 180, step)
        az += list(a)
        el += [e] * len(a)
    az.append(0), el.append(90)
    return np.array(az, np.int64), np.array(el, np.int64)


def grid_vectors(step):
    """the grid's unit vectors (x, y, z): computed in float64, rounded to float32 -- the table every path reads"""
    az, el = doa_grid(step)
    return np.ascontiguousarray(_unit(az, el), np.float32)


def mic_matrix():
    """D^-1 in float64, D the 3 x 3 matrix of rows p_m - p_0 (m = 1 .. 3), p = MIC_RADIUS x the tetrahedron's capsule directions"""
    from .rooms import _capsule_units
    p = MIC_RADIUS * _capsule_units()
    return np.linalg.inv(p[1:] - p[:1])


class DoaResult:
    """count int32 (B, Fl), n_votes int32 (B, Fl), cell int32 (B, Fl, K), score float32 (B, Fl, K), direction float32 (B, Fl, K, 3)
    unit vectors (x, y, z), spectrum float32 (B, Fl, G) or None -- tensors on the features' device; unused slots hold -1 / +0.0."""

    def __init__(self, count, n_votes, cell, score, direction, spectrum=None):
        self.count, self.n_votes, self.cell, self.score, self.direction, self.spectrum = count, n_votes, cell, score, direction, spectrum

    def numpy(self):
        """the same arrays on the host, as numpy"""
        to = lambda t: None if t is None else t.detach().cpu().numpy()
        return DoaResult(*(to(getattr(self, f)) for f in ('count', 'n_votes', 'cell', 'score', 'direction', 'spectrum')))


class DoaHistogram:
    """The localiser for one feature configuration.  audio_format 'foa' | 'mic'; feature_type 'salsa' | 'salsa_lite' ('salsa_ipd' has
    no frequency normalisation and is refused).  fs, n_fft, fmin_doa, fmax_doa: as the features were extracted (fmax_doa None: 9000 foa,
    4000 mic, 2000 salsa_lite); they place the columns.  fmin_hz / fmax_hz narrow the voting bins (None: all of them, but for MIC fmax_hz
    defaults to 1600 Hz, below which the phase differences do not wrap on either baffle); as for the extractor's own limits the upper bin
    floor(fmax_hz n_fft / fs) is excluded.  grid_step (degrees) divides 90; kernel_deg the cap's half width; max_sources <= 8;
    suppress_deg >= 1; min_score > 0; frames_per_label feature frames per label frame; norm_range the accepted vote lengths."""

    def __init__(self, audio_format='foa', feature_type='salsa', fs=24000, n_fft=512, fmin_doa=50, fmax_doa=None, fmin_hz=None,
                 fmax_hz=None, grid_step=5, kernel_deg=15.0, max_sources=2, suppress_deg=30.0, min_score=8.0, frames_per_label=8,
                 norm_range=(0.5, 2.0)):
        if audio_format not in _lib.FORMAT:
            raise ValueError('audio_format must be foa or mic')
        if feature_type not in ('salsa', 'salsa_lite'):
            raise ValueError("feature_type is 'salsa' or 'salsa_lite': salsa_ipd's phase differences are not normalised by frequency")
        if feature_type == 'salsa_lite' and audio_format != 'mic':
            raise ValueError('salsa_lite is the mic format\'s')
        if fmax_doa is None:
            fmax_doa = 2000 if feature_type == 'salsa_lite' else (9000 if audio_format == 'foa' else 4000)
        self.audio_format, self.feature_type = audio_format, feature_type
        self.grid_step, self.max_sources, self.frames_per_label = int(grid_step), int(max_sources), int(frames_per_label)
        self.azimuth, self.elevation = doa_grid(self.grid_step)
        self.grid = grid_vectors(self.grid_step)
        if not 1 <= self.max_sources <= MAX_SOURCES:
            raise ValueError('1 .. %d sources' % MAX_SOURCES)
        if not (0.0 < kernel_deg < 90.0 and 1.0 <= suppress_deg <= 180.0 and min_score > 0.0 and self.frames_per_label >= 1):
            raise ValueError('0 < kernel_deg < 90, 1 <= suppress_deg <= 180, min_score > 0, frames_per_label >= 1')
        self.norm_lo, self.norm_hi = (float(np.float32(v)) for v in norm_range)
        if not 0.0 < self.norm_lo <= self.norm_hi < 1e38:
            raise ValueError('norm_range is (lo, hi) with 0 < lo <= hi')
        lower, upper, _ = bin_limits(fs, n_fft, fmin_doa, fmax_doa)
        if audio_format == 'mic' and fmax_hz is None:
            fmax_hz = MIC_FMAX_HZ
        b0 = lower if fmin_hz is None else max(lower, int(np.ceil(float(fmin_hz) * n_fft / fs)))
        b1 = upper if fmax_hz is None else min(upper, int(np.floor(float(fmax_hz) * n_fft / fs)))
        if b1 <= b0:
            raise ValueError('no DOA bin between fmin_hz and fmax_hz')
        self.col0, self.col1 = b0 - lower, b1 - lower
        if self.frames_per_label * (self.col1 - self.col0) > MAX_VOTES:
            raise ValueError('%d frames x %d columns: more than %d cells per label frame' % (self.frames_per_label, self.col1 - self.col0,
                                                                                            MAX_VOTES))
        self.kernel_deg, self.suppress_deg = float(kernel_deg), float(suppress_deg)
        c0 = np.float32(np.cos(np.deg2rad(self.kernel_deg)))
        self.c0, self.inv = float(c0), float(np.float32(1.0 / (1.0 - np.float64(c0))))
        self.cos_suppress = float(np.float32(np.cos(np.deg2rad(self.suppress_deg))))
        self.min_score = float(np.float32(min_score))
        self.matrix = np.ascontiguousarray(mic_matrix(), np.float32) if audio_format == 'mic' else None
        self._dev = {}

    n_cells = property(lambda self: len(self.grid))

    def _grid_on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.grid).to(device)
        return self._dev[key]

    def _check(self, features):
        if not (torch.is_tensor(features) and features.dtype == torch.float32 and features.dim() == 4 and features.is_contiguous()):
            raise ValueError('features: a contiguous float32 tensor (B, C >= 7, T, F), time-major')
        B, Cf, T, F = features.shape
        if Cf < 7 or B < 1 or self.col1 > F or T < self.frames_per_label:
            raise ValueError('features (B, C >= 7, T >= %d, F >= %d) expected, got %s' % (self.frames_per_label, self.col1, tuple(features.shape)))
        return B, Cf, T, F, T // self.frames_per_label

    def localize(self, features, spectrum=False):
        """features float32 (B, C >= 7, T, F), as SalsaExtractor.extract and the feature bank hold them -> DoaResult.  A CUDA tensor goes
        to the HIP kernel (one launch on the current stream, nothing synchronised), a CPU tensor -- or any, under SALSA_HIP_DOA=0 -- to
        the composed torch path."""
        B, Cf, T, F, Fl = self._check(features)
        if features.is_cuda and HIP_DOA:
            return self._localize_hip(features, bool(spectrum), B, Cf, T, F, Fl)
        return self._localize_torch(features, bool(spectrum), B, Fl)

    __call__ = localize

    # ------------------------------------------------------------------------------------------------------------- the kernel
    def _localize_hip(self, x, spectrum, B, Cf, T, F, Fl):
        K, G, dev = self.max_sources, self.n_cells, x.device
        if not _lib.load().salsa_doa_hist_supported(Cf, F, self.col0, self.col1, self.frames_per_label, self.grid_step, K):
            raise ValueError('salsa_doa_hist does not take this shape: %s' % ((Cf, F, self.col0, self.col1, self.frames_per_label, K),))
        count = torch.empty((B, Fl), dtype=torch.int32, device=dev)
        votes = torch.empty((B, Fl), dtype=torch.int32, device=dev)
        cell = torch.empty((B, Fl, K), dtype=torch.int32, device=dev)
        score = torch.empty((B, Fl, K), dtype=torch.float32, device=dev)
        direction = torch.empty((B, Fl, K, 3), dtype=torch.float32, device=dev)
        spec = torch.empty((B, Fl, G), dtype=torch.float32, device=dev) if spectrum else None
        res = DoaResult(count, votes, cell, score, direction, spec)
        self.launch(x, res)
        return res

    def launch(self, x, res):
        """salsa_doa_hist on x into the caller's tensors of `res` (spectrum may be None), on x's device and its current stream"""
        L, grid = _lib.load(), self._grid_on(x.device)
        B, Cf, T, F = x.shape
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        M = self.matrix.ctypes.data_as(C.c_void_p) if self.matrix is not None else None
        with torch.cuda.device(x.device):
            rc = L.salsa_doa_hist(ptr(x), B, Cf, T, F, self.col0, self.col1, self.frames_per_label, _lib.FORMAT[self.audio_format], M,
                                  ptr(grid), self.grid_step, self.c0, self.inv, self.cos_suppress, self.min_score, self.norm_lo, self.norm_hi,
                                  self.max_sources, ptr(res.count), ptr(res.n_votes), ptr(res.cell), ptr(res.score), ptr(res.direction),
                                  ptr(res.spectrum), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
        if rc:
            raise RuntimeError('salsa_doa_hist failed (%d): %s' % (rc, _lib.last_error()))

    # ------------------------------------------------------------------------------------------------------------- composed torch
    def _localize_torch(self, x, spectrum, B, Fl):
        """The definition composed from torch calls, a chunk of label frames at a time.  Gated cells stay in place with a zero term, so
        the cumulative sums along the cell axis add the votes in vote order (x + 0 is exact)."""
        K, G, P, dev = self.max_sources, self.n_cells, self.frames_per_label, x.device
        U = self._grid_on(dev)                                                                  # (G, 3)
        ncol = self.col1 - self.col0
        n = P * ncol
        v = x[:, 4:7, :Fl * P, self.col0:self.col1].reshape(B, 3, Fl, n).permute(0, 2, 3, 1).reshape(B * Fl, n, 3)
        count = torch.zeros(B * Fl, dtype=torch.int32, device=dev)
        votes = torch.zeros(B * Fl, dtype=torch.int32, device=dev)
        cell = torch.full((B * Fl, K), -1, dtype=torch.int32, device=dev)
        score = torch.zeros((B * Fl, K), dtype=torch.float32, device=dev)
        direction = torch.zeros((B * Fl, K, 3), dtype=torch.float32, device=dev)
        spec = torch.zeros((B * Fl, G), dtype=torch.float32, device=dev) if spectrum else None
        M = torch.from_numpy(self.matrix).to(dev) if self.matrix is not None else None
        cells = torch.arange(G, device=dev)
        step = max(1, TORCH_ELEMENTS // (n * G))
        for lo in range(0, B * Fl, step):
            w = v[lo:lo + step]                                                                 # (Fc, n, 3)
            ok = torch.isfinite(w).all(dim=-1) & (w != 0).any(dim=-1)
            w = torch.where(ok[..., None], w, torch.zeros_like(w))
            u = w @ M.T if M is not None else w[..., [2, 0, 1]]
            length = torch.sqrt((u * u).sum(dim=-1))
            ok = ok & (length >= self.norm_lo) & (length <= self.norm_hi)
            u = torch.where(ok[..., None], u / length[..., None], torch.zeros_like(u))
            term = torch.clamp_min((u @ U.T - self.c0) * self.inv, 0.0) * ok[..., None]         # (Fc, n, G)
            s = torch.cumsum(term, dim=1)[:, -1]                                                # (Fc, G)
            del term
            votes[lo:lo + step] = ok.sum(dim=1).to(torch.int32)
            if spec is not None:
                spec[lo:lo + step] = s
            alive = torch.ones(len(w), dtype=torch.bool, device=dev)
            free = torch.ones_like(s, dtype=torch.bool)
            for k in range(K):
                masked = torch.where(free, s, torch.full_like(s, -1.0))
                best = masked.max(dim=1).values
                g = torch.where(masked == best[:, None], cells[None, :], G).min(dim=1).values.clamp_max(G - 1)      # the lowest index of a tie
                alive = alive & (best >= self.min_score)
                Ug = U[g]                                                                       # (Fc, 3)
                inside = ok & ((u * Ug[:, None, :]).sum(dim=-1) >= self.c0)
                m = torch.cumsum(u * inside[..., None], dim=1)[:, -1]
                d = m / torch.sqrt((m * m).sum(dim=-1, keepdim=True))
                sl = slice(lo, lo + len(w))
                cell[sl, k] = torch.where(alive, g.to(torch.int32), torch.full_like(g, -1, dtype=torch.int32))
                score[sl, k] = torch.where(alive, best, torch.zeros_like(best))
                direction[sl, k] = torch.where(alive[:, None], d, torch.zeros_like(d))
                count[sl] += alive.to(torch.int32)
                free = free & ~((Ug @ U.T) >= self.cos_suppress)
        return DoaResult(count.view(B, Fl), votes.view(B, Fl), cell.view(B, Fl, K), score.view(B, Fl, K), direction.view(B, Fl, K, 3),
                         spec.view(B, Fl, G) if spec is not None else None)

    # ------------------------------------------------------------------------------------------------------------- rows
    def rows(self, result, class_id=0):
        """The DCASE rows (frame, class, track k, azimuth, elevation) of every clip, a list of int64 (n, 5) arrays sorted by frame and
        track.  Integer degrees, rounded on the host in float64 from the refined direction (azimuth 180 is written -180).  With every
        ground-truth class mapped to class_id they go to the host scorers as they are."""
        r = result.numpy() if torch.is_tensor(result.count) else result
        out = []
        for b in range(r.count.shape[0]):
            f, k = np.nonzero(np.arange(r.cell.shape[2])[None, :] < r.count[b][:, None])
            az, el = direction_degrees(r.direction[b, f, k])
            az, el = np.rint(az).astype(np.int64), np.rint(el).astype(np.int64)
            az = np.where(az >= 180, az - 360, az)
            out.append(np.stack([f, np.full_like(f, int(class_id)), k, az, el], axis=1).astype(np.int64).reshape(-1, 5))
        return out


def direction_degrees(d):
    """(azimuth, elevation) in degrees, float64, of unit vectors (..., 3)"""
    d = np.asarray(d, np.float64)
    return np.rad2deg(np.arctan2(d[..., 1], d[..., 0])), np.rad2deg(np.arcsin(np.clip(d[..., 2], -1.0, 1.0)))


def _assign(cost):
    """the minimum-cost assignment of min(rows, columns) pairs of a small cost matrix -> [(row, column), ...], by dynamic programming
    over column subsets (at most 8 columns)"""
    cost = np.asarray(cost, np.float64)
    if cost.shape[0] > cost.shape[1]:
        return [(r, c) for c, r in _assign(cost.T)]
    R, Cn = cost.shape
    best = {0: (0.0, [])}
    for r in range(R):
        nxt = {}
        for used, (tot, pairs) in best.items():
            for c in range(Cn):
                if not (used >> c) & 1:
                    cand = (tot + cost[r, c], pairs + [(r, c)])
                    if (used | 1 << c) not in nxt or cand[0] < nxt[used | 1 << c][0]:
                        nxt[used | 1 << c] = cand
        best = nxt
    return min(best.values(), key=lambda t: t[0])[1]


class AngularErrors:
    """errors float64 (n,): the matched pairs' angles in degrees, with clip and frame int64 (n,) of each; missed / extra: ground-truth
    directions without a peak and peaks without a ground truth, summed over the n_frames label frames compared"""

    def __init__(self, errors, clip, frame, missed, extra, n_frames):
        self.errors, self.clip, self.frame = np.asarray(errors, np.float64), np.asarray(clip, np.int64), np.asarray(frame, np.int64)
        self.missed, self.extra, self.n_frames = int(missed), int(extra), int(n_frames)


def angular_errors(result, scenes_or_rows, label_rate=10, fs=24000):
    """Peaks against ground truth, label frame by label frame.  scenes_or_rows: a scenes.Scenes (its scene_rows are taken per clip) or
    one (n, 5) row array per clip (frame, class, track, azimuth, elevation; classes are ignored).  Per frame the peaks and the
    ground-truth directions are matched by the minimum-cost assignment (cost: the angle between them); the rest count as missed or
    extra.  Frames at or past the result's label frames are dropped."""
    from . import scenes as sc
    r = result.numpy() if torch.is_tensor(result.count) else result
    B, Fl = r.count.shape
    rows = [sc.scene_rows(scenes_or_rows[b], label_rate, fs) for b in range(B)] if isinstance(scenes_or_rows, sc.Scenes) else list(scenes_or_rows)
    if len(rows) != B:
        raise ValueError('one set of rows per clip')
    errors, clip, frame, missed, extra = [], [], [], 0, 0
    for b in range(B):
        gt = np.asarray(rows[b], np.int64).reshape(-1, 5)
        gt = gt[gt[:, 0] < Fl]
        order = np.argsort(gt[:, 0], kind='stable')
        gt = gt[order]
        starts = np.searchsorted(gt[:, 0], np.arange(Fl + 1))
        vec = _unit(gt[:, 3], gt[:, 4]).reshape(-1, 3)
        for f in range(Fl):
            g = vec[starts[f]:starts[f + 1]]
            e = np.asarray(r.direction[b, f, :r.count[b, f]], np.float64)
            if len(g) and len(e):
                ang = np.rad2deg(np.arccos(np.clip(e @ g.T, -1.0, 1.0)))
                pairs = _assign(ang)
                errors += [ang[i, j] for i, j in pairs]
                clip += [b] * len(pairs)
                frame += [f] * len(pairs)
            missed += max(0, len(g) - len(e))
            extra += max(0, len(e) - len(g))
    return AngularErrors(errors, clip, frame, missed, extra, B * Fl)
