"""On-device counterpart of the reference's data layer (dataset/database.py + dataset/dataloader.py) for training
straight from raw audio (BASELINE.json config 4) or from a tree of precomputed feature files (config 3; add_feature_files +
load_feature_scaler = Database.load_chunk_data / load_feature_scaler): clips are extracted on the GPU, kept there in the reference's
concatenated ``(C, sum T, F)`` layout (database.py:230-231), normalised on load with the scaler (the first 4 channels for
SALSA, every channel for the baseline IV / GCC features, whose scaler holds all C: :197-202) and sliced into chunks with the
reference's segment index arithmetic (:98-119).  ``__getitem__`` returns the same 4-tuple contract as SeldDataset
(dataloader.py:37-62) minus augmentation: (X (C,chunk,F), sed, doa, name).

Nothing here runs in DataLoader worker processes: HIP contexts do not survive fork, so extraction happens on the
training process' stream (SURVEY.md section 7 'hard parts')."""
import os

import numpy as np
import torch

from . import _lib
from .extractor import SalsaExtractor, normalize_, scaler_accumulate, scaler_finish


def second2frame(second: float, fs: int, hop_len: int) -> int:
    """database.py:75-81"""
    return int(round(int(second * fs) / hop_len))


def get_segment_idxes(n_frames: int, chunk_len: int, chunk_hop_len: int, downsample_ratio: int, pointer: int):
    """database.py:98-119 verbatim semantics: chunk start indices (at the segment rate) + the advanced pointer."""
    assert n_frames % downsample_ratio == 0, 'n_features_frames is not divisible by downsample ratio'
    n_crop = n_frames // downsample_ratio
    cl, ch = chunk_len // downsample_ratio, chunk_hop_len // downsample_ratio
    assert cl <= n_crop, 'Number of cropped frame is less than chunk len'
    idxes = np.arange(pointer, pointer + n_crop - cl + 1, ch).tolist()
    if (n_crop - cl) % ch != 0:
        idxes.append(pointer + n_crop - cl)             # include the leftover of the cropped data
    return idxes, pointer + n_crop


def sort_tracks(track_number: np.ndarray) -> np.ndarray:
    """database.py:242-251: track ids from the shortest to the longest track (row counts; ids without rows count 0)."""
    n_tracks = int(np.max(track_number)) + 1
    durations = np.zeros((n_tracks,), dtype=np.int32)
    for itrack in range(n_tracks):
        durations[itrack] = np.sum(track_number == itrack)
    return np.argsort(durations)


def load_classwise_gt(gt_meta_fn, n_frames: int, n_classes: int = 12, label_upsample_ratio: int = 8,
                      output_format: str = 'reg_xyz'):
    """Database.load_classwise_gt (dataset/database.py:253-296): a DCASE2021 metadata CSV -- rows
    ``frame_number, sound_class_idx, track_number, azimuth, elevation`` at the 10-Hz label rate, no header -- to the training
    targets of a clip of ``n_frames`` FEATURE frames: sed (n_label_frames, n_classes) float32 in {0, 1} and doa (n_label_frames,
    3 * n_classes) float32 = [x | y | z] unit vectors of the active classes, zeros elsewhere.  Tracks are written from the
    shortest to the longest (:268, :275), rows of a track in file order, so where two tracks hold the same class in the same
    frame the LONGER track's direction stays (and a later row of one track overrides an earlier one).  The trigonometry runs
    in float32 on the float32 radian arrays, as the reference's numpy does (:285-291).  CPU / numpy: a clip has a few thousand
    rows."""
    import pandas as pd
    assert n_frames % label_upsample_ratio == 0, 'mismatch ground truth and feature frame rate'
    if output_format not in ('reg_xyz', 'accdoa'):
        raise ValueError('doa output format {} is not valid'.format(output_format))
    n_label_frames = n_frames // label_upsample_ratio
    df = pd.read_csv(gt_meta_fn, header=None, names=['frame_number', 'sound_class_idx', 'track_number', 'azimuth', 'elevation'])
    frame_number, sound_class_idx, track_number = df['frame_number'].values, df['sound_class_idx'].values, df['track_number'].values
    azimuth, elevation = df['azimuth'].values, df['elevation'].values
    sed = np.zeros((n_label_frames, n_classes), dtype=np.float32)
    azi = np.zeros((n_label_frames, n_classes), dtype=np.float32)
    ele = np.zeros((n_label_frames, n_classes), dtype=np.float32)
    if len(df):
        # one fancy assignment in the reference's write order (tracks shortest first, file order inside a track): numpy keeps the
        # LAST value written to a repeated index, which is what the reference's nested loops leave behind
        rank = np.empty(int(np.max(track_number)) + 1, dtype=np.int64)
        rank[sort_tracks(track_number)] = np.arange(len(rank))
        order = np.argsort(rank[track_number.astype(np.int64)], kind='stable')
        fr, cl = frame_number[order].astype(np.int64), sound_class_idx[order].astype(np.int64)
        sed[fr, cl] = 1.0
        azi[fr, cl] = azimuth[order] * np.pi / 180.0
        ele[fr, cl] = elevation[order] * np.pi / 180.0
    x, y, z = np.cos(azi) * np.cos(ele), np.sin(azi) * np.cos(ele), np.sin(ele)
    off = sed < 1
    x[off] = 0.0
    y[off] = 0.0
    z[off] = 0.0
    return sed, np.concatenate((x, y, z), axis=-1)


def load_trackwise_gt(gt_meta_fn, n_frames: int, n_classes: int = 12, label_upsample_ratio: int = 8, n_slots: int = 3):
    """The Multi-ACCDOA targets of a clip (the reference has none): the CSV and the float32 trigonometry of
    load_classwise_gt, but same-class overlaps are KEPT.  Per (frame, class) the distinct tracks present are ordered from the longest
    track to the shortest (row counts over the file, sort_tracks reversed; ties: the lower track id first) and fill slots 0, 1, ..
    n_slots - 1, so the active slots are always a prefix; further tracks are dropped.  Within one track the last row in file order
    wins, as in load_classwise_gt.  -> sed (n_label_frames, n_slots * n_classes) in {0, 1}, doa (n_label_frames, 3 * n_slots *
    n_classes) = [x | y | z] blocks with slot n of class c at column n * n_classes + c of each block, and n_dropped, the number of
    (frame, class, track) entries that found no slot.  Without same-class overlaps slot 0 is load_classwise_gt's result bit for
    bit."""
    import pandas as pd
    assert n_frames % label_upsample_ratio == 0, 'mismatch ground truth and feature frame rate'
    if n_slots < 1:
        raise ValueError('n_slots must be positive')
    n_label_frames = n_frames // label_upsample_ratio
    df = pd.read_csv(gt_meta_fn, header=None, names=['frame_number', 'sound_class_idx', 'track_number', 'azimuth', 'elevation'])
    frame_number, sound_class_idx = df['frame_number'].values.astype(np.int64), df['sound_class_idx'].values.astype(np.int64)
    track_number = df['track_number'].values.astype(np.int64)
    azi_rad, ele_rad = df['azimuth'].values * np.pi / 180.0, df['elevation'].values * np.pi / 180.0
    nc = n_slots * n_classes
    sed = np.zeros((n_label_frames, nc), dtype=np.float32)
    azi = np.zeros((n_label_frames, nc), dtype=np.float32)
    ele = np.zeros((n_label_frames, nc), dtype=np.float32)
    n_dropped = 0
    if len(df):
        if sound_class_idx.min() < 0 or sound_class_idx.max() >= n_classes or frame_number.min() < 0 or frame_number.max() >= n_label_frames:
            raise IndexError('a metadata row lies outside %d label frames x %d classes' % (n_label_frames, n_classes))
        durations = np.bincount(track_number)
        cells = {}
        for i in range(len(df)):                                               # the last row of a (frame, class, track) stays
            cells.setdefault((frame_number[i], sound_class_idx[i]), {})[track_number[i]] = i
        for (fr, cl), tracks in cells.items():
            ranked = sorted(tracks, key=lambda t: (-durations[t], t))
            n_dropped += max(0, len(ranked) - n_slots)
            for slot, t in enumerate(ranked[:n_slots]):
                col, i = slot * n_classes + cl, tracks[t]
                sed[fr, col] = 1.0
                azi[fr, col] = azi_rad[i]
                ele[fr, col] = ele_rad[i]
    x, y, z = np.cos(azi) * np.cos(ele), np.sin(azi) * np.cos(ele), np.sin(ele)
    off = sed < 1
    x[off] = 0.0
    y[off] = 0.0
    z[off] = 0.0
    return sed, np.concatenate((x, y, z), axis=-1), n_dropped


LABEL_FORMATS = ('classwise', 'trackwise')


class GpuFeatureBank(torch.utils.data.Dataset):
    """extractor: a SalsaExtractor, a baseline_features.BaselineExtractor, or None (precomputed feature files).
    n_scaler_channels: the channels fit_scaler() covers and finalize() normalises; None takes it from the data -- every channel
    of a BaselineExtractor's output (the reference's baseline compute_scaler, feature_extraction.py:526-586), else 4 (SALSA).
    A scaler given by load_feature_scaler / set_scaler normalises its own number of channels, (4 | C, 1, F).
    label_format: 'classwise' (gt_meta= is read by load_classwise_gt) or 'trackwise' (Multi-ACCDOA, DESIGN.md section 9i: n_classes
    = 3 x the real classes, gt_meta= is read by load_trackwise_gt, n_dropped counts what found no slot); sed= / doa= arrays are
    taken as they are under both."""

    def __init__(self, extractor: SalsaExtractor = None, fs=24000, hop_len=300, label_rate=10, chunk_len_s=8.0,
                 chunk_hop_len_s=0.5, n_classes=12, max_clip_s=60, device=None, n_scaler_channels=None, label_format='classwise'):
        if label_format not in LABEL_FORMATS:
            raise ValueError('invalid label_format %r (supported: %s)' % (label_format, ', '.join(LABEL_FORMATS)))
        if label_format == 'trackwise' and n_classes % 3 != 0:
            raise ValueError("label_format 'trackwise' holds three slots per class: n_classes = 3 x the real classes, not %d" % n_classes)
        self.label_format = label_format
        self.n_dropped = 0                                                     # trackwise: (frame, class, track) entries beyond three slots
        self.ex = extractor                                                    # None: a bank of precomputed feature files (add_feature_files)
        self.n_scaler_channels = n_scaler_channels
        self.device = extractor.device if extractor is not None else torch.device(device if device is not None else 'cuda')
        self.fs, self.hop_len, self.label_rate, self.n_classes = fs, hop_len, label_rate, n_classes
        self.chunk_len = second2frame(chunk_len_s, fs, hop_len)
        self.chunk_hop_len = second2frame(chunk_hop_len_s, fs, hop_len)
        self.upsample = int((fs / hop_len) / label_rate)                       # feature frames per label frame (8)
        self.max_frames = int(max_clip_s * label_rate) * self.upsample         # "make sure we have 4800 frames" (:205-207)
        self.blocks, self.names, self.chunk_idx, self.chunk_name = [], [], [], []
        self.clip_start, self.clip_len = [], []                               # every clip's first frame in the bank and its frames
        self.sed, self.doa, self.gt_idx = [], [], []
        self.pointer = self.gt_pointer = 0
        self.features = None
        self.mean = self.std = None
        self._sums, self._n = None, 0

    # -------------------------------------------------------------------------------------------- ingest
    def add_clips(self, audio, names, sed=None, doa=None, gt_meta=None):
        """audio: float32 [B,4,N] (numpy or CUDA tensor).  Labels, one of: ``gt_meta`` = per-clip paths of DCASE metadata CSVs
        (read by load_classwise_gt, as Database.load_chunk_data does, database.py:209-211); ``sed`` / ``doa`` = per-clip label
        arrays at label rate, (T_lab, n_classes) and (T_lab, 3*n_classes); none of them -> zeros (inference)."""
        assert self.ex is not None, 'this bank was built without an extractor: it takes feature files only'
        a = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio, np.float32))
        self._ingest(self.ex.extract(a.to(self.ex.device).contiguous()), names, sed, doa, gt_meta)

    def add_feature_files(self, feature_files, names=None, sed=None, doa=None, gt_meta=None):
        """PRECOMPUTED features (BASELINE config 3; what extract_features() wrote: a 'feature' dataset (7, T, F) per clip) instead of
        audio -- Database.load_chunk_data's file loop (database.py:190-207: read, trim to max_nframes_per_file * label_upsample_ratio
        frames; the normalisation of :197-202 happens in finalize(), on the device).  Clips of one shape go to the device in one copy."""
        from . import io as sio
        names = [os.path.splitext(os.path.basename(f))[0] for f in feature_files] if names is None else list(names)
        assert len(names) == len(feature_files)
        arrays = [np.ascontiguousarray(sio.load_arrays(f)['feature'], np.float32) for f in feature_files]
        i = 0
        while i < len(arrays):                                                 # runs of equal shape, file order kept (the pointers are sequential)
            j = i + 1
            while j < len(arrays) and arrays[j].shape == arrays[i].shape:
                j += 1
            feats = torch.from_numpy(np.stack(arrays[i:j])).to(self.device)
            sl = slice(i, j)
            self._ingest(feats, names[sl], None if sed is None else sed[sl], None if doa is None else doa[sl],
                         None if gt_meta is None else gt_meta[sl])
            i = j

    def load_feature_scaler(self, scaler_file):
        """<fmt>_feature_scaler.h5 -> the bank's scaler: Database.load_feature_scaler (database.py:87-96: 'mean', 'std' of shape
        (4, 1, F) for SALSA, (C, 1, F) for the baseline features -- then every channel is normalised, :197-202)"""
        from . import io as sio
        z = sio.load_arrays(scaler_file)
        self.set_scaler(z['mean'], z['std'])
        return self.mean, self.std

    def add_features(self, feats, names, sed=None, doa=None, gt_meta=None):
        """Feature tensors float32 [B,C,T,F] as they are (labels as add_clips takes them).  The scaler's sums and the normalisation
        are HIP kernels, so a bank on the CPU -- what the composed torch path of batch_augmented and the CPU suite work on -- holds
        features that are normalised already and is closed with finalize(normalize=False)."""
        self._ingest(feats.to(self.device), names, sed, doa, gt_meta)

    def _ingest(self, feats, names, sed=None, doa=None, gt_meta=None):
        assert gt_meta is None or (sed is None and doa is None), 'give either metadata CSVs or label arrays'
        n_frames = min(feats.shape[2], self.max_frames)
        n_frames -= n_frames % self.upsample
        feats = feats[:, :, :n_frames].contiguous()
        if self.n_scaler_channels is None:
            from .baseline_features import BaselineExtractor
            self.n_scaler_channels = feats.shape[1] if isinstance(self.ex, BaselineExtractor) else 4
        if feats.is_cuda:                                                      # (a CPU bank: add_features)
            self._sums = scaler_accumulate(feats, self._sums, self.n_scaler_channels)
        self._n += feats.shape[0] * n_frames
        if gt_meta is not None:
            assert len(gt_meta) == len(names)
            if self.label_format == 'trackwise':
                labels = [load_trackwise_gt(fn, n_frames, self.n_classes // 3, self.upsample) for fn in gt_meta]
                self.n_dropped += sum(lab[2] for lab in labels)
            else:
                labels = [load_classwise_gt(fn, n_frames, self.n_classes, self.upsample) for fn in gt_meta]
            sed, doa = [lab[0] for lab in labels], [lab[1] for lab in labels]
        for i, name in enumerate(names):
            self.clip_start.append(self.pointer)
            self.clip_len.append(n_frames)
            idxes, self.pointer = get_segment_idxes(n_frames, self.chunk_len, self.chunk_hop_len, 1, self.pointer)
            gidx, self.gt_pointer = get_segment_idxes(n_frames, self.chunk_len, self.chunk_hop_len, self.upsample,
                                                      self.gt_pointer)
            assert len(idxes) == len(gidx), 'nchunks for sed and gt are different'
            self.blocks.append(feats[i])
            self.names.append(name)
            self.chunk_idx += idxes
            self.gt_idx += gidx
            self.chunk_name += [name] * len(idxes)
            n_lab = n_frames // self.upsample
            dev = feats.device
            self.sed.append(torch.zeros(n_lab, self.n_classes, device=dev) if sed is None
                            else torch.as_tensor(sed[i][:n_lab], dtype=torch.float32, device=dev))
            self.doa.append(torch.zeros(n_lab, 3 * self.n_classes, device=dev) if doa is None
                            else torch.as_tensor(doa[i][:n_lab], dtype=torch.float32, device=dev))
        self.features = None

    def fit_scaler(self):
        """scaler over everything ingested so far (the reference fits it on all dev files)."""
        self.mean, self.std = scaler_finish(self._sums, self._n)
        return self.mean, self.std

    def set_scaler(self, mean, std):
        self.mean, self.std = torch.as_tensor(np.asarray(mean, np.float32)), torch.as_tensor(np.asarray(std, np.float32))

    def finalize(self, normalize=True):
        """concatenate along time (database.py:230) and normalise the scaler's channels in place (normalize=False: the features
        are normalised already, add_features)."""
        assert self.mean is not None or not normalize, 'call fit_scaler() or set_scaler() first'
        feats = torch.cat(self.blocks, dim=1).contiguous()                   # (C, sum T, F)
        if normalize:
            normalize_(feats[None], self.mean, self.std)
        self.features = feats
        self.sed_all, self.doa_all = torch.cat(self.sed), torch.cat(self.doa)
        self.blocks = []
        return self

    # -------------------------------------------------------------------------------------------- Dataset
    def __len__(self):
        return len(self.chunk_idx)

    def __getitem__(self, i):
        assert self.features is not None, 'call finalize() first'
        s, g = self.chunk_idx[i], self.gt_idx[i]
        x = self.features[:, s:s + self.chunk_len]
        n_lab = self.chunk_len // self.upsample
        return x, self.sed_all[g:g + n_lab], self.doa_all[g:g + n_lab], self.chunk_name[i]

    def batch(self, indices):
        xs, ss, ds, ns = zip(*(self[i] for i in indices))
        return torch.stack(xs), torch.stack(ss), torch.stack(ds), list(ns)

    # -------------------------------------------------------------------------------------------- one-call batches
    def _fused(self):
        """the one switch of the hand-written batch path: CUDA banks go through salsa_bank_batch unless SALSA_BANK_BATCH=0"""
        return self.features.is_cuda and os.environ.get('SALSA_BANK_BATCH', '1') != '0'

    def _check_indices(self, indices):
        """host integers, checked here: the kernel trusts the starts it is handed"""
        idx = [int(i) for i in (indices.tolist() if hasattr(indices, 'tolist') else indices)]
        if not idx:
            raise ValueError('an empty batch')
        n = len(self.chunk_idx)
        for i in idx:
            if not 0 <= i < n:
                raise IndexError('chunk index %d outside the bank of %d chunks' % (i, n))
        return idx

    def batch_augmented(self, indices, draws=None, audio_format='foa', feature_type='salsa'):
        """The training batch of chunks ``indices`` (host integers) with the drawn augmentation ``draws`` (augment.draw_augment's dict;
        None: no augmentation) of the recipe of (audio_format, feature_type): x (B,C,T,F), sed (B,L,nc), doa (B,L,3 nc) with the target
        half of the swap, names.  On a CUDA bank this is ONE call of libsalsa_hip.so (salsa_bank_batch: gather, augment and label in at
        most three launches, no stacked copy, no host synchronisation); on a CPU bank, or with SALSA_BANK_BATCH=0, the composed path --
        batch(), then augment.apply_augment_hip (CPU: apply_augment_torch), then augment.swap_targets -- whose result it equals bit for
        bit."""
        from . import augment as aug
        assert self.features is not None, 'call finalize() first'
        idx = self._check_indices(indices)
        swap, _, n_zero, _ = aug.recipe(audio_format, feature_type)
        Cn, n_bank, F = self.features.shape
        if Cn != (10 if swap == 'gcc' else 7):
            raise ValueError('the %s recipe takes %d channels, the bank has %d' % (swap, 10 if swap == 'gcc' else 7, Cn))
        B, T, L = len(idx), self.chunk_len, self.chunk_len // self.upsample
        names = [self.chunk_name[i] for i in idx]
        if draws is not None and any(tuple(draws[k].shape[:1]) != (B,) for k in ('m', 'shift', 'up', 'top', 'h', 'left', 'w', 'u')):
            raise ValueError('draws for another batch size than %d' % B)
        if not self._fused():
            x, sed, doa, _ = self.batch(idx)
            if draws is None:
                return x, sed, doa, names
            if not x.is_cuda:
                x, doa = aug.apply_augment_torch(x, doa, draws, audio_format, self.n_classes, feature_type)
                return x, sed, doa, names
            m_dev = draws['m'].pin_memory().to(x.device, non_blocking=True)
            return (aug.apply_augment_hip(x, draws, audio_format, feature_type), sed,
                    aug.swap_targets(doa, m_dev, 'foa' if swap == 'foa' else 'mic', self.n_classes), names)
        starts, gts = [self.chunk_idx[i] for i in idx], [self.gt_idx[i] for i in idx]
        if min(starts) < 0 or max(starts) + T > n_bank or min(gts) < 0 or max(gts) + L > self.sed_all.shape[0]:
            raise IndexError('a chunk window lies outside the bank')
        # ONE pinned staging buffer, one copy: starts and gt starts (int64), the 40 parameters and the 8 fill draws of every sample
        host = torch.empty(52 * B, dtype=torch.int32, pin_memory=True)
        host[:4 * B].view(torch.int64).copy_(torch.tensor([starts, gts], dtype=torch.int64).reshape(-1))
        par, u = host[4 * B:44 * B].view(B, 40), host[44 * B:].view(torch.float32).view(B, 8)
        has_rects = False
        if draws is None:
            par.zero_()
            u.zero_()
        else:
            par.zero_()
            par[:, 0:4] = draws['m']
            par[:, 4], par[:, 5] = draws['shift'], draws['up']
            par[:, 8:16], par[:, 16:24], par[:, 24:32], par[:, 32:40] = draws['top'], draws['h'], draws['left'], draws['w']
            u.copy_(draws['u'].float())
            has_rects = bool(((draws['h'] > 0) & (draws['w'] > 0)).any())    # (FOA SALSA draws none: no min / max launch)
        dev = self.features.device
        staged = host.to(dev, non_blocking=True)
        x = torch.empty((B, Cn, T, F), dtype=torch.float32, device=dev)
        sed = torch.empty((B, L, self.n_classes), dtype=torch.float32, device=dev)
        doa = torch.empty((B, L, 3 * self.n_classes), dtype=torch.float32, device=dev)
        ws = torch.empty((B, 2), dtype=torch.int32, device=dev) if has_rects else None
        rec = _lib.BANK_RECIPE[swap if draws is not None else 'none']
        base = staged.data_ptr()
        self._bank_call(x, sed, doa, base, base + 8 * B, B, T, L, rec, n_zero or 0, base + 16 * B, base + 176 * B, has_rects, ws)
        return x, sed, doa, names

    def _bank_call(self, x, sed, doa, p_start, p_gt, B, T, L, rec, n_zero, p_par, p_u, has_rects, ws):
        import ctypes as C
        Cn, n_bank, F = self.features.shape
        dev = self.features.device
        vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)      # noqa: E731
        labels = sed is not None
        with torch.cuda.device(dev):
            rc = _lib.load().salsa_bank_batch(
                vp(self.features), Cn, n_bank, F, vp(self.sed_all if labels else None), vp(self.doa_all if labels else None),
                self.sed_all.shape[0], self.n_classes, C.c_void_p(p_start), C.c_void_p(p_gt if labels else None), B, T, L, rec, n_zero,
                C.c_void_p(p_par), C.c_void_p(p_u), int(has_rects), vp(x), vp(sed), vp(doa), vp(ws),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc:
            raise RuntimeError('salsa_bank_batch failed: ' + _lib.last_error())

    def clip_batch(self, lo, hi):
        """Whole clips lo..hi-1 as one tensor (hi - lo, C, T, F) -- what infer_pipelined's featurize hands the model -- through the
        same call with the recipe 'none' (CPU bank or SALSA_BANK_BATCH=0: stacked slices).  The clips must be equally long."""
        assert self.features is not None, 'call finalize() first'
        if not 0 <= lo < hi <= len(self.clip_start):
            raise IndexError('clips %d..%d of a bank of %d' % (lo, hi, len(self.clip_start)))
        T = self.clip_len[lo]
        if any(n != T for n in self.clip_len[lo:hi]):
            raise ValueError('clips %d..%d differ in length: %s' % (lo, hi, sorted(set(self.clip_len[lo:hi]))))
        starts = self.clip_start[lo:hi]
        if min(starts) < 0 or max(starts) + T > self.features.shape[1]:
            raise IndexError('a clip window lies outside the bank')
        if not self._fused():
            return torch.stack([self.features[:, s:s + T] for s in starts])
        dev = self.features.device
        staged = torch.tensor(starts, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        x = torch.empty((hi - lo, self.features.shape[0], T, self.features.shape[2]), dtype=torch.float32, device=dev)
        self._bank_call(x, None, None, staged.data_ptr(), None, hi - lo, T, max(1, T // self.upsample), _lib.BANK_RECIPE['none'], 0,
                        None, None, False, None)
        return x


def _mix_seed(*parts):
    """one 63-bit generator seed from a tuple of small integers (seed, epoch, step, rank): a fixed arithmetic, so any step's draws can
    be replayed from its coordinates"""
    h = 0x9E3779B97F4A7C15
    for p in parts:
        h = ((h ^ (int(p) & 0xFFFFFFFFFFFFFFFF)) * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        h ^= h >> 31
    return h & 0x7FFFFFFFFFFFFFFF


class BankLoader:
    """The epochs of the reference's ``DataLoader(train_dataset, batch_size, shuffle=True)`` (dataset/datamodule.py) over a finalized
    GpuFeatureBank, without workers: a seeded permutation per epoch, batches of ``batch_size`` with the short last one kept (the
    reference has no drop_last), ``train_fraction`` as Lightning's limit_train_batches (experiments/train.py:53), and per step one
    batch_augmented call with draws from a generator seeded by (seed, epoch, step, rank).  ``rank`` / ``world`` split the permutation
    as torch's DistributedSampler does: padded by wrapping to a multiple of ``world``, then every world-th index from ``rank``, so all
    ranks take the same number of steps.  Items: (x, sed, doa, names) plus ``indices`` and ``draws`` when asked for."""

    def __init__(self, bank, batch_size=32, seed=2021, audio_format='foa', feature_type='salsa', augment=True, train_fraction=1.0,
                 rank=0, world=1, with_indices=False, with_draws=False):
        if batch_size < 1 or world < 1 or not 0 <= rank < world or not 0.0 <= train_fraction <= 1.0:
            raise ValueError('BankLoader: bad batch_size, rank / world or train_fraction')
        if len(bank) == 0:
            raise ValueError('BankLoader: the bank holds no chunk')
        self.bank, self.batch_size, self.seed = bank, int(batch_size), int(seed)
        self.audio_format, self.feature_type, self.augment = audio_format, feature_type, augment
        self.train_fraction, self.rank, self.world = train_fraction, rank, world
        self.with_indices, self.with_draws = with_indices, with_draws
        n_rank = -(-len(bank) // world)
        self.n_batches = -(-n_rank // self.batch_size)
        self.steps_per_epoch = int(self.n_batches * train_fraction)

    def __len__(self):
        return self.steps_per_epoch

    def epoch_indices(self, epoch):
        """the permutation of epoch ``epoch`` (all ranks')"""
        return torch.randperm(len(self.bank), generator=torch.Generator().manual_seed(self.seed + int(epoch)))

    def rank_indices(self, epoch):
        """this rank's share of the permutation (world 1: all of it)"""
        perm = self.epoch_indices(epoch)
        if self.world == 1:
            return perm
        total = -(-len(perm) // self.world) * self.world
        while len(perm) < total:                                               # (wrap: DistributedSampler's padding)
            perm = torch.cat([perm, perm[:total - len(perm)]])
        return perm[self.rank:total:self.world]

    def step_indices(self, epoch, step):
        return self.rank_indices(epoch)[step * self.batch_size:(step + 1) * self.batch_size]

    def step_draws(self, epoch, step, batch):
        """the augmentation draws of one step, None with augment=False"""
        if not self.augment:
            return None
        from .augment import draw_augment
        gen = torch.Generator().manual_seed(_mix_seed(self.seed, epoch, step, self.rank))
        return draw_augment(batch, self.bank.chunk_len, self.bank.features.shape[2], self.audio_format, gen,
                            feature_type=self.feature_type)

    def epoch(self, epoch, first_step=0):
        """the items of one epoch from step ``first_step`` on"""
        mine = self.rank_indices(epoch)
        for step in range(first_step, self.steps_per_epoch):
            idx = mine[step * self.batch_size:(step + 1) * self.batch_size]
            draws = self.step_draws(epoch, step, len(idx))
            item = self.bank.batch_augmented(idx, draws, self.audio_format, self.feature_type)
            if self.with_indices:
                item = item + (idx,)
            if self.with_draws:
                item = item + (draws,)
            yield item
