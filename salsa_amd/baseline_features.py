"""Drop-in Python surface of the reference's baseline features (dataset/feature_extraction.py): log-mel / log-linear
spectrograms with the intensity vector (FOA) or GCC-PHAT (MIC), computed by the HIP kernels of
salsa_amd/csrc/baseline_kernels.hip behind include/salsa_baseline.h.

  reference                                                  here
  MelSpecExtractor / MelSpecIvExtractor / MelSpecGccExtractor  same names, ``.extract(audio (C, N)) -> (C', T, F)``
  LinSpecIvExtractor / LogSpecGccExtractor                     same names
  select_extractor(feature_type, ...)           :486-523       select_extractor
  compute_scaler(feature_dir, audio_format)     :526-594       compute_scaler ('mean', 'std', 'scalar_mean', 'scalar_std')
  extract_features(data_config, feature_type, task, is_compressed_freq)  :597-693   extract_features
                                                               (+ ``python -m salsa_amd.baseline_features --name=value``)
  (device-resident, batched)                                   BaselineExtractor: torch [B, 4, N] -> [B, C, T, F]

``.extract`` returns float32 for every type.  The reference returns float64 for the GCC types (its irfft output) but writes
float32 to its feature files; the values agree to float32 round-off.  n_fft must be 256 or 512 for every type (the
reference's mel types accept other sizes; this port refuses them).  There is no CPU path.
"""
import ctypes as C
import os
import sys
from timeit import default_timer as timer

import numpy as np
import yaml

from . import _lib
from . import io as sio
from .features import _cli, _extract_serial, _rmtree_parallel, _torch

import logging  # noqa: E402
_log = logging.getLogger('salsa_amd.baseline_features')

FEATURE_TYPES = tuple(_lib.BASELINE_FEATURE)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))       # GCC channels 4..9: gcc_phat(sig=audio[m], refsig=audio[n])


def _raise(rc):
    msg = _lib.last_error()
    if rc == _lib.E_NFFT:
        raise AssertionError(msg)
    if rc == _lib.E_INVAL:
        raise ValueError(msg)
    raise RuntimeError('libsalsa_hip: %s (code %d)' % (msg, rc))


def mel_matrix(fs, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr=fs, n_fft, n_mels, fmin, fmax) of librosa 0.8.0 (float32 (n_mels, n_fft//2 + 1)), host code"""
    W = np.zeros((int(n_mels), int(n_fft) // 2 + 1), np.float32)
    rc = _lib.load().salsa_baseline_mel_matrix(int(fs), int(n_fft), int(n_mels), float(fmin), float(fmax or 0.0),
                                               W.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        _raise(rc)
    return W


def n_output_channels(feature_type):
    return 10 if feature_type.endswith('gcc') else 7 if feature_type.endswith('iv') else 4


def lin_freqs(n_fft, is_compressed_freq=True):
    """rows of the log-linear types (extract_features :631-639)"""
    assert n_fft == 256 or n_fft == 512, 'nfft = {} is not supported'.format(n_fft)
    return (200 if n_fft == 512 else 100) if is_compressed_freq else n_fft // 2


def output_shape(feature_type, n_samples, n_fft=512, hop_length=300, n_mels=128, is_compressed_freq=True):
    """(C, T, F) of one clip"""
    if feature_type not in FEATURE_TYPES:
        raise NotImplementedError('Feature type {} is not implemented!'.format(feature_type))
    F = lin_freqs(n_fft, is_compressed_freq) if feature_type.startswith('lin') else int(n_mels)
    return n_output_channels(feature_type), 1 + int(n_samples) // int(hop_length), F


def gcc_lags(L, n2):
    """indices into the n2-point cross-correlation of the L kept lags: cc[-L//2:] ++ cc[:L//2] (:113, :440)"""
    return np.concatenate((np.arange(n2)[-L // 2:], np.arange(n2)[:L // 2]))


class BaselineExtractor:
    """Batched, device-resident extraction of one baseline feature type on one MI355X: float32 CUDA [B, 4, N] planar ->
    float32 [B, C, T, F].  Keyword names follow the reference's YAML ``data`` block."""

    def __init__(self, feature_type='linspeciv', fs=24000, n_fft=512, hop_len=300, win_len=None, n_mels=128, fmin=50,
                 fmax=None, is_compressed_freq=True, device=None):
        if feature_type not in FEATURE_TYPES:
            raise NotImplementedError('Feature type {} is not implemented!'.format(feature_type))
        torch = _torch()
        self.L = _lib.load()
        self.feature_type = feature_type
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        self.params = _lib.BaselineParams(fs=int(fs), n_fft=int(n_fft), hop_len=int(hop_len), win_len=int(win_len or n_fft),
                                          n_mels=int(n_mels), feature_type=_lib.BASELINE_FEATURE[feature_type], fmin=float(fmin),
                                          fmax=float(fmax or 0.0), is_compressed_freq=int(bool(is_compressed_freq)), reserved=0)
        self._plan = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.L.salsa_baseline_plan_create(C.byref(self.params), C.byref(self._plan))
        if rc:
            self._plan = None
            _raise(rc)

    def __del__(self):
        if getattr(self, '_plan', None):
            self.L.salsa_baseline_plan_destroy(self._plan)
            self._plan = None

    def output_shape(self, n_samples):
        c, t, f = C.c_int(), C.c_int64(), C.c_int()
        rc = self.L.salsa_baseline_output_shape(self._plan, int(n_samples), C.byref(c), C.byref(t), C.byref(f))
        if rc:
            _raise(rc)
        return c.value, t.value, f.value

    def extract(self, audio, out=None):
        """audio float32 CUDA [B, 4, N] (planar) -> features float32 [B, C, T, F] (into ``out`` if given)"""
        torch = _torch()
        assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 3 and audio.is_contiguous()
        B, ch, N = audio.shape
        assert ch == 4, 'the baseline features are defined for 4-channel clips'
        if audio.device != self.device:
            raise ValueError('plan is bound to %s, audio is on %s' % (self.device, audio.device))
        shape = (B,) + self.output_shape(N)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=audio.device)
        else:
            assert tuple(out.shape) == shape and out.dtype == torch.float32 and out.is_contiguous() and out.device == audio.device
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            rc = self.L.salsa_baseline_extract_batch(self._plan, C.c_void_p(audio.data_ptr()), B, N, C.c_void_p(out.data_ptr()),
                                                     None, 0, stream)
        if rc:
            _raise(rc)
        return out

    __call__ = extract


class _NumpyFront:
    """``.extract(audio (C, N)) -> (C', T, F)`` float32 numpy through a lazily built BaselineExtractor"""
    feature_type = None

    def _kw(self):
        raise NotImplementedError

    def extract(self, audio_input: np.ndarray) -> np.ndarray:
        torch = _torch()
        if getattr(self, '_ex', None) is None:
            self._ex = BaselineExtractor(feature_type=self.feature_type, **self._kw())
        a = np.ascontiguousarray(audio_input, np.float32)
        n_ch = a.shape[0]
        if self.feature_type != 'melspec':
            assert n_ch == 4, '{} is defined for 4-channel clips'.format(self.feature_type)
        outs = []
        for c0 in range(0, n_ch, 4):                       # melspec: any channel count, in groups of 4 (silent padding)
            blk = a[c0:c0 + 4]
            if blk.shape[0] < 4:
                blk = np.concatenate([blk, np.zeros((4 - blk.shape[0], a.shape[1]), np.float32)])
            o = self._ex.extract(torch.from_numpy(np.ascontiguousarray(blk[None])).to(self._ex.device))[0].cpu().numpy()
            outs.append(o if self.feature_type != 'melspec' else o[:min(4, n_ch - c0)])
        return np.concatenate(outs, axis=0)


class FeatureExtractor(_NumpyFront):
    """Base of the mel types (:21-51): melW = librosa.filters.mel(sr=fs, n_fft, n_mels, fmin, fmax)."""

    def __init__(self, fs: int, n_fft: int, hop_length: int, n_mels: int, win_length: int = None, fmin: int = 50,
                 fmax: int = None, window: str = 'hann'):
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.window = window
        self.win_length = self.n_fft if win_length is None else win_length
        assert self.win_length <= self.n_fft, 'Windown length is greater than nfft!'
        if window != 'hann':
            raise ValueError('only the hann window of the reference configs is implemented')
        if n_fft not in (256, 512):
            raise NotImplementedError('n_fft = {}: the GPU path supports n_fft 256 and 512 only'.format(n_fft))
        self.fs, self.n_mels, self.fmin, self.fmax = fs, n_mels, fmin, fmax
        self.melW = mel_matrix(fs, n_fft, n_mels, fmin, fmax)
        self._ex = None

    def _kw(self):
        return dict(fs=self.fs, n_fft=self.n_fft, hop_len=self.hop_length, win_len=self.win_length, n_mels=self.n_mels,
                    fmin=self.fmin, fmax=self.fmax)


class MelSpecExtractor(FeatureExtractor):
    """log-mel spectrograms (n_channels, T, n_mels) (:224-267)"""
    feature_type = 'melspec'


class MelSpecIvExtractor(FeatureExtractor):
    """log-mel + intensity vector through melW, (7, T, n_mels) (:159-221)"""
    feature_type = 'melspeciv'


class MelSpecGccExtractor(FeatureExtractor):
    """log-mel + GCC-PHAT, (10, T, n_mels) (:54-156)"""
    feature_type = 'melspecgcc'


class LinSpecIvExtractor(_NumpyFront):
    """log-linear + intensity vector, (7, T, 200 | 100 | n_fft/2) (:270-359)"""
    feature_type = 'linspeciv'

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
        self.n_freqs = lin_freqs(n_fft, is_compress_high_freq)
        self.W = compress_matrix(n_fft, is_compress_high_freq)
        self._ex = None

    def _kw(self):
        return dict(n_fft=self.n_fft, hop_len=self.hop_length, win_len=self.win_length,
                    is_compressed_freq=self.is_compress_high_freq)


class LogSpecGccExtractor(LinSpecIvExtractor):
    """log-linear + GCC-PHAT, (10, T, 200 | 100 | n_fft/2) (:362-483)"""
    feature_type = 'linspecgcc'


def select_extractor(feature_type: str, fs: int, n_fft: int, hop_length: int, n_mels: int, win_length: int = None,
                     fmin: int = 50, fmax: int = None):
    """:486-523 (the lin types compress when n_mels < n_fft // 2)"""
    if feature_type == 'melspec':
        return MelSpecExtractor(fs=fs, n_fft=n_fft, hop_length=hop_length, n_mels=n_mels, win_length=win_length, fmin=fmin, fmax=fmax)
    if feature_type == 'melspeciv':
        return MelSpecIvExtractor(fs=fs, n_fft=n_fft, hop_length=hop_length, n_mels=n_mels, win_length=win_length, fmin=fmin, fmax=fmax)
    if feature_type == 'melspecgcc':
        return MelSpecGccExtractor(fs=fs, n_fft=n_fft, hop_length=hop_length, n_mels=n_mels, win_length=win_length, fmin=fmin, fmax=fmax)
    if feature_type == 'linspeciv':
        return LinSpecIvExtractor(n_fft=n_fft, hop_length=hop_length, win_length=win_length, is_compress_high_freq=(n_mels < n_fft // 2))
    if feature_type == 'linspecgcc':
        return LogSpecGccExtractor(n_fft=n_fft, hop_length=hop_length, win_length=win_length, is_compress_high_freq=(n_mels < n_fft // 2))
    raise NotImplementedError('Feature type {} is not implemented!'.format(feature_type))


def feature_description(feature_type, fs, n_fft, hop_length, n_mels, is_compressed_freq=True):
    """-> (directory name, n_mels | n_freqs) of extract_features (:631-645)"""
    if feature_type in ('linspeciv', 'linspecgcc'):
        assert n_fft == 256 or n_fft == 512, 'nfft = {} is not supported for {}'.format(n_fft, feature_type)
        n_mels = lin_freqs(n_fft, is_compressed_freq)
        return '{}fs_{}nfft_{}nhop_{}nfreqs'.format(fs, n_fft, hop_length, n_mels), n_mels
    return '{}fs_{}nfft_{}nhop_{}nmels'.format(fs, n_fft, hop_length, n_mels), n_mels


def scaler_stats(features):
    """(mean (C,1,F), std (C,1,F), scalar_mean (C,1,1), scalar_std (C,1,1)) float32 of an iterable of (C, T, F) arrays: per channel
    and frequency over all frames, and per channel over all (frame, frequency) values; population std (StandardScaler.var_).
    Sums in float64 around the first array's means (conditioning of the one-pass variance)."""
    n = 0
    for f in features:
        d64 = np.asarray(f, np.float64)
        if n == 0:
            shift = d64.mean(axis=1)                            # (C, F)
            s, ss = np.zeros_like(shift), np.zeros_like(shift)
            sshift = d64.mean(axis=(1, 2))                      # (C,)
            s1, ss1 = np.zeros_like(sshift), np.zeros_like(sshift)
        d = d64 - shift[:, None, :]
        s += d.sum(axis=1)
        ss += (d * d).sum(axis=1)
        e = d64 - sshift[:, None, None]
        s1 += e.sum(axis=(1, 2))
        ss1 += (e * e).sum(axis=(1, 2))
        n += d64.shape[1]
        F = d64.shape[2]
    mean = shift + s / n
    std = np.sqrt(np.maximum(ss / n - (s / n) ** 2, 0.0))
    smean = sshift + s1 / (n * F)
    sstd = np.sqrt(np.maximum(ss1 / (n * F) - (s1 / (n * F)) ** 2, 0.0))
    f32 = lambda x: np.asarray(x, np.float32)
    return f32(mean[:, None, :]), f32(std[:, None, :]), f32(smean[:, None, None]), f32(sstd[:, None, None])


def compute_scaler(feature_dir: str, audio_format: str) -> str:
    """:526-594: the scaler over every file of <audio_format>_dev, all C channels -> <feature_dir>/<fmt>_feature_scaler.h5
    with 'mean', 'std' (C,1,F) and 'scalar_mean', 'scalar_std' (C,1,1), float32.  Returns the path written."""
    start_time = timer()
    train_feature_dir = os.path.join(feature_dir, audio_format + '_dev')
    fns = sio.feature_files(train_feature_dir)
    mean, std, smean, sstd = scaler_stats(sio.load_arrays(os.path.join(train_feature_dir, fn))['feature'] for fn in fns)
    written = sio.save_arrays(os.path.join(feature_dir, audio_format + '_feature_scaler.h5'), mean=mean, std=std,
                              scalar_mean=smean, scalar_std=sstd)
    _log.info('scaler: %d files -> %s (%.3f s)', len(fns), written, timer() - start_time)
    return written


def extract_features(data_config: str = 'configs/tnsse2021_feature_config.yml', feature_type: str = 'linspeciv',
                     task: str = 'feature_scaler', is_compressed_freq: bool = True, batch_size: int = 32) -> None:
    """:597-693: features of every clip of <format>_dev and <format>_eval into
    <feature_dir>/<feature_type>/<fs>fs_<n_fft>nfft_<hop>nhop_<n>nfreqs|nmels/<split>/ (cleared first; sorted file order;
    a (C, T, F) float32 'feature' per clip), then the scaler.  ``batch_size`` (clips per device call) is the only extra argument."""
    with open(data_config, 'r') as stream:
        cfg = yaml.safe_load(stream)
    d = cfg['data']
    audio_format, fs, n_fft, hop_length, win_length = d['format'], d['fs'], d['n_fft'], d['hop_len'], d['win_len']
    fmin, fmax, n_mels = d['fmin'], d['fmax'], d['n_mels']
    fmax = np.min((fmax, fs // 2))
    desc, n_mels = feature_description(feature_type, fs, n_fft, hop_length, n_mels, is_compressed_freq)
    _log.info('feature description: %s', desc)
    if feature_type not in FEATURE_TYPES:
        raise NotImplementedError('Feature type {} is not implemented!'.format(feature_type))
    if audio_format not in ('foa', 'mic'):
        raise ValueError('Unknown audio format {}'.format(audio_format))
    if task in ['feature_scaler', 'feature']:
        ex = BaselineExtractor(feature_type=feature_type, fs=fs, n_fft=n_fft, hop_len=hop_length, win_len=win_length,
                               n_mels=n_mels, fmin=fmin, fmax=float(fmax), is_compressed_freq=is_compressed_freq)
        for split in (audio_format + '_dev', audio_format + '_eval'):
            start_time = timer()
            audio_dir = os.path.join(cfg['data_dir'], split)
            feature_dir = os.path.join(cfg['feature_dir'], feature_type, desc, split)
            _rmtree_parallel(feature_dir)
            os.makedirs(feature_dir, exist_ok=True)
            _extract_serial(ex, list(enumerate(sorted(os.listdir(audio_dir)))), audio_dir, feature_dir, fs, batch_size)
            _log.info('split %s: %.3f s', split, timer() - start_time)
    if task in ['feature_scaler', 'scaler']:
        compute_scaler(feature_dir=os.path.join(cfg['feature_dir'], feature_type, desc), audio_format=audio_format)


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(message)s')
    _cli(extract_features, sys.argv[1:])
