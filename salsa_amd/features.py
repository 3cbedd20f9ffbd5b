"""Drop-in Python surface of the reference's full-SALSA module (dataset/salsa_feature_extraction.py): same function
names, arguments, defaults, exceptions and file layout, with the arithmetic running in libsalsa_hip.so on an MI355X.

  reference                                             here
  extract_normalized_eigenvector(X, ...)   :17-129      extract_normalized_eigenvector  (numpy in / numpy out)
  MagStftExtractor(...).W / .extract       :132-201     MagStftExtractor
  compute_scaler(feature_dir, audio_format) :204-262    compute_scaler
  extract_features(data_config, ...)       :265-391     extract_features  (+ ``python -m salsa_amd.features --flag=...``)

There is no CPU path: without a GPU / without the built library these functions raise.
"""
import os
import shutil
import sys
from timeit import default_timer as timer

import numpy as np
import yaml

from . import io as sio
from .file_pipeline import SLOT_CLIPS, ScalerSums, _FilePipeline, pcm_to_planar, pipeline_for, release_file_pipelines  # noqa: F401
from .io import feature_name

import logging  # noqa: E402
_log = logging.getLogger('salsa_amd.features')


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('salsa_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback')
    return torch


def extract_normalized_eigenvector(X, condition_number: float = 5.0, n_hopframes: int = 3, is_tracking: bool = True,
                                   audio_format: str = 'foa', fs: int = None, n_fft: int = None,
                                   lower_bin: int = None):
    """X <np.ndarray (n_bins, n_frames, n_chans=4)> clipped spectrogram -> (3, n_bins, n_frames) float64.
    Mirrors dataset/salsa_feature_extraction.py:17 (values are taken at complex64 precision, which is what the
    reference's STFT holds)."""
    if audio_format not in ('foa', 'mic'):
        raise ValueError('audio format {} is not valid'.format(audio_format))
    torch = _torch()
    from .extractor import SalsaExtractor
    X = np.asarray(X)
    assert X.ndim == 3 and X.shape[2] == 4, 'X must be (n_bins, n_frames, 4)'
    # (the plan's own DOA band is irrelevant here: the band is whatever rows X holds)
    ex = SalsaExtractor(fs=fs or 24000, n_fft=n_fft or 512, hop_len=300, fmin_doa=0, fmax_doa=(fs or 24000) // 8,
                        cond_num=condition_number, n_hopframes=n_hopframes, is_tracking=is_tracking,
                        audio_format=audio_format)
    Xd = torch.from_numpy(np.ascontiguousarray(X.astype(np.complex64))[None]).cuda()
    out = ex.eigvec(Xd, lower_bin=int(lower_bin or 0))
    return out[0].cpu().numpy()


class MagStftExtractor:
    """Log-linear spectrograms (n_channels, n_timesteps, 200|100|n_fft/2).  Mirrors :132-201."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int = None, window: str = 'hann',
                 is_compress_high_freq: bool = True):
        from .extractor import compress_matrix
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.window = window
        self.win_length = self.n_fft if win_length is None else win_length
        assert self.win_length <= self.n_fft, 'Windown length is greater than nfft!'
        assert n_fft == 512 or n_fft == 256, 'nfft is not 512 or 256'
        if window != 'hann':
            raise ValueError('only the hann window of the reference configs is implemented')
        self.is_compress_high_freq = is_compress_high_freq
        self.W = compress_matrix(n_fft, is_compress_high_freq)
        self._ex = None

    def extract(self, audio_input: np.ndarray) -> np.ndarray:
        torch = _torch()
        from .extractor import SalsaExtractor
        if self._ex is None:
            self._ex = SalsaExtractor(n_fft=self.n_fft, hop_len=self.hop_length, win_len=self.win_length,
                                      is_compress_high_freq=self.is_compress_high_freq)
        a = np.ascontiguousarray(audio_input, np.float32)
        n_ch = a.shape[0]
        outs = []
        for c0 in range(0, n_ch, 4):                       # the kernel works on groups of 4 channels
            blk = a[c0:c0 + 4]
            if blk.shape[0] < 4:
                blk = np.concatenate([blk, np.zeros((4 - blk.shape[0], a.shape[1]), np.float32)])
            o = self._ex.logspec(torch.from_numpy(np.ascontiguousarray(blk[None])).cuda())[0].cpu().numpy()
            outs.append(o[:min(4, n_ch - c0)])
        return np.concatenate(outs, axis=0)


def compute_scaler(feature_dir: str, audio_format: str) -> None:
    """Mean / std of the 4 spectrogram channels over ALL files of <audio_format>_dev -> <audio_format>_feature_scaler
    (datasets 'mean', 'std', shape (4,1,F) float32).  Mirrors :204-262 (StandardScaler.partial_fit: population std)."""
    _log.info('scaler: streaming mean / std over %s_dev', audio_format)
    start_time = timer()
    train_feature_dir = os.path.join(feature_dir, audio_format + '_dev')
    feature_fn_list = sio.feature_files(train_feature_dir)
    afeature = sio.load_arrays(os.path.join(train_feature_dir, feature_fn_list[0]))['feature']
    n_channels = afeature.shape[0]
    assert n_channels == 7, 'only support n_channels = 7, got {}'.format(n_channels)
    n_feature_channels = 4
    shift = afeature[:n_feature_channels].astype(np.float64).mean(axis=1)     # conditioning of the one-pass variance
    n, s, ss = 0, np.zeros_like(shift), np.zeros_like(shift)
    for feature_fn in feature_fn_list:
        afeature = sio.load_arrays(os.path.join(train_feature_dir, feature_fn))['feature']
        d = afeature[:n_feature_channels].astype(np.float64) - shift[:, None, :]
        s += d.sum(axis=1)
        ss += (d * d).sum(axis=1)
        n += afeature.shape[1]
    feature_mean = (shift + s / n)[:, None, :]
    feature_std = np.sqrt(np.maximum(ss / n - (s / n) ** 2, 0.0))[:, None, :]
    scaler_path = os.path.join(feature_dir, audio_format + '_feature_scaler.h5')
    written = sio.save_arrays(scaler_path, mean=feature_mean, std=feature_std)
    _log.info('scaler: %d files x %s -> %s', len(feature_fn_list), afeature.shape, written)
    _log.info('scaler: %.3f s', timer() - start_time)


def write_scaler_from_sums(feature_dir: str, audio_format: str, sums, n_frames: int) -> str:
    """compute_scaler's result from statistics accumulated on the device while the dev split was extracted: mean = sum / n,
    std = sqrt(sum of squares / n - mean^2) (population, like StandardScaler.var_), both (4,1,F) float32 -> the scaler file."""
    h = sums.detach().cpu().numpy()
    mean = h[0] / n_frames
    std = np.sqrt(np.maximum(h[1] / n_frames - mean * mean, 0.0))
    scaler_path = os.path.join(feature_dir, audio_format + '_feature_scaler.h5')
    written = sio.save_arrays(scaler_path, mean=mean[:, None, :].astype(np.float32), std=std[:, None, :].astype(np.float32))
    _log.info('scaler: from the device statistics of %d frames -> %s', n_frames, written)
    return written


def _parse(data_config):
    with open(data_config, 'r') as stream:
        cfg = yaml.safe_load(stream)
    d = cfg['data']
    return cfg, d['format'], d['fs'], d['n_fft'], d['hop_len'], d['win_len'], d['fmin_doa'], d['fmax_doa']


def tree_layout(feature_type, audio_format, fs, n_fft, hop_len, cond_num, fmax_doa, is_tracking=True, is_compress_high_freq=True):
    """-> (description, (dev split, eval split)) of the reference's tree <feature_dir>/<feature_type>/<audio_format>/<description>/<split>/
    (:290-301 for 'salsa'; salsa_lite_feature_extraction.py:69, no ``cond`` field and no suffixes, for 'salsa_lite' / 'salsa_ipd')."""
    if feature_type == 'salsa':
        desc = '{}fs_{}nfft_{}nhop_{}cond_{}fmaxdoa'.format(fs, n_fft, hop_len, int(cond_num), int(fmax_doa))
        desc += '' if is_tracking else '_notracking'
        desc += '' if is_compress_high_freq else '_nocompress'
    else:
        desc = '{}fs_{}nfft_{}nhop_{}fmaxdoa'.format(fs, n_fft, hop_len, int(fmax_doa))
    return desc, (audio_format + '_dev', audio_format + '_eval')


USE_FILE_PIPELINE = os.environ.get('SALSA_FILE_PIPELINE', '1') != '0'
RAW_PCM = os.environ.get('SALSA_RAW_PCM', '1') != '0'     # plain PCM WAV clips: upload the file's bytes, convert on the device (0: decode on the host)
FUSED_SCALER = os.environ.get('SALSA_FUSED_SCALER', '1') != '0'   # task='feature_scaler': the scaler from device statistics (0: re-read the files)


def _rmtree_parallel(path, threads: int = 8):
    """shutil.rmtree(path, ignore_errors=True) with the directory's own files unlinked from a few threads first: emptying last run's
    split folder (:344) is freeing 27 MB of page cache / tmpfs per clip, 2.5 ms each from one thread -- twice what extracting the
    clip takes (tools/probes/harness_profile.py)."""
    try:
        files = [e.path for e in os.scandir(path) if e.is_file(follow_symlinks=False)]
    except OSError:
        files = []
    if len(files) > 2 * threads:
        from concurrent.futures import ThreadPoolExecutor

        def rm(p):
            try:
                os.unlink(p)
            except OSError:
                pass
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(rm, files))
    shutil.rmtree(path, ignore_errors=True)


def _extract_serial(ex, todo, audio_dir, feature_dir, fs, batch_size):
    """Load, batch by length, extract and write the clips todo = [(count, file name)] one device call at a time.  ``ex`` needs only
    ``.device`` and ``.extract(batch)`` (salsa_amd.baseline_features runs its extractor through here)."""
    torch = _torch()
    pending = {}                                            # n_samples -> [(count, fn, audio)]

    def flush(items):
        batch = np.stack([a for _, _, a in items])
        feats = ex.extract(torch.from_numpy(batch).to(ex.device)).cpu().numpy()
        for (count, fn, _), f in zip(items, feats):
            sio.save_arrays(os.path.join(feature_dir, feature_name(fn)), feature=f)
            _log.debug('clip %d %s -> %s', count, fn, f.shape)

    for count, audio_fn in todo:
        audio_input = sio.load_audio(os.path.join(audio_dir, audio_fn), sr=fs, device=ex.device)
        assert audio_input.shape[0] == 4, '{}: expected a 4-channel clip'.format(audio_fn)
        lst = pending.setdefault(audio_input.shape[1], [])
        lst.append((count, audio_fn, audio_input))
        if len(lst) == batch_size:
            flush(lst)
            lst.clear()
    for lst in pending.values():
        if lst:
            flush(lst)


def _extract_split(ex, audio_dir, feature_dir, fs, batch_size, shard=None, clear=True, stats=None, scaler=None):
    """Extract the clips of one split directory, batching clips of equal length (one device round trip per batch, overlapped
    with its neighbours' and with the file reads / writes: salsa_amd.file_pipeline).  scaler: a ScalerSums for the split's statistics.
    shard = (rank, world): this process takes a contiguous range of the sorted file list (salsa_amd.distributed)."""
    torch = _torch()
    if clear:
        _rmtree_parallel(feature_dir)                       # the reference empties the split's folder first (:344)
    os.makedirs(feature_dir, exist_ok=True)
    todo = list(enumerate(sorted(os.listdir(audio_dir))))
    if shard is not None:
        from .distributed import shard_range
        lo, hi = shard_range(len(todo), *shard)
        todo = todo[lo:hi]
    if USE_FILE_PIPELINE and todo:
        pipe = pipeline_for(ex)
        with pipe.lock, torch.cuda.device(ex.device):
            pipe.run(todo, audio_dir, feature_dir, fs, batch_size, stats, scaler, raw_pcm=RAW_PCM, slot_clips=SLOT_CLIPS)
        return
    if scaler is not None:
        scaler.available = False                            # (serial loop / empty split: compute_scaler reads the files, as the reference does)
    _extract_serial(ex, todo, audio_dir, feature_dir, fs, batch_size)


def _extract_splits(ex, cfg, root, splits, task, batch_size, shard=None):
    """The split loop of every extract_features: the clips of <data_dir>/<split> -> <root>/<split>, each folder emptied first.  Returns
    the scaler statistics taken on the device while <format>_dev was extracted (:214-215), or None when ``task`` / FUSED_SCALER do not
    ask for them.  shard = (rank, world) of a torch.distributed job: rank 0 empties the folders, a barrier lets the others in."""
    sums = ScalerSums() if (task == 'feature_scaler' and FUSED_SCALER) else None
    for split in splits:
        _log.info('split %s: extracting on %s', split, ex.device)
        start_time = timer()
        feature_dir = os.path.join(root, split)
        if shard is not None:
            if shard[0] == 0:
                _rmtree_parallel(feature_dir)
                os.makedirs(feature_dir, exist_ok=True)
            if shard[1] > 1:
                import torch.distributed as dist
                dist.barrier()
        _extract_split(ex, os.path.join(cfg['data_dir'], split), feature_dir, cfg['data']['fs'], batch_size, shard=shard,
                       clear=shard is None, scaler=sums if split.endswith('_dev') else None)
        _log.info('split %s: done in %.3f s', split, timer() - start_time)
    return sums


def extract_features(data_config: str = 'configs/tnsse2021_salsa_feature_config.yml',
                     cond_num: float = 5,
                     n_hopframes: int = 3,
                     is_tracking: bool = True,
                     is_compress_high_freq: bool = True,
                     task: str = 'feature_scaler',
                     batch_size: int = 32) -> None:
    """Extract salsa features (log-linear spectrogram + normalized eigenvector) for every clip of <format>_dev and
    <format>_eval, then the scaler.  Mirrors :265-391 (same directory naming, split iteration, sorted file order,
    (7,T,F) float32 'feature' per clip).  ``batch_size`` (clips per device call) is the only extra argument."""
    cfg, audio_format, fs, n_fft, hop_length, win_length, fmin_doa, fmax_doa = _parse(data_config)
    feature_type = 'salsa'
    fmax_doa = int(np.min((fmax_doa, fs // 2)))
    assert n_fft == 512 or n_fft == 256, 'only 256 or 512 fft is supported'
    feature_description, splits = tree_layout(feature_type, audio_format, fs, n_fft, hop_length, cond_num, fmax_doa,
                                              is_tracking, is_compress_high_freq)
    if audio_format not in ('foa', 'mic'):
        raise ValueError('Unknown audio format {}'.format(audio_format))
    _log.info('feature directory name: %s', feature_description)
    root = os.path.join(cfg['feature_dir'], feature_type, audio_format, feature_description)
    if task in ['feature_scaler', 'feature']:
        from .extractor import SalsaExtractor
        ex = SalsaExtractor(fs=fs, n_fft=n_fft, hop_len=hop_length, win_len=win_length, fmin_doa=fmin_doa,
                            fmax_doa=fmax_doa, cond_num=cond_num, n_hopframes=n_hopframes, is_tracking=is_tracking,
                            is_compress_high_freq=is_compress_high_freq, audio_format=audio_format)
        sums = _extract_splits(ex, cfg, root, splits, task, batch_size)
        if sums is not None and sums.available:
            write_scaler_from_sums(root, audio_format, sums.sums, sums.n_frames)
            return
    if task in ['feature_scaler', 'scaler']:
        compute_scaler(feature_dir=root, audio_format=audio_format)


def _cli(fn, argv):
    """python-fire style ``--name=value`` flags -> keyword arguments (the reference wraps the function in fire.Fire)."""
    kw = {}
    for a in argv:
        assert a.startswith('--') and '=' in a, 'use --name=value'
        k, v = a[2:].split('=', 1)
        kw[k] = yaml.safe_load(v)
    fn(**kw)


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(message)s')      # progress lines on the console, as a CLI should
    _cli(extract_features, sys.argv[1:])


