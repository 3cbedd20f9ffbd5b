"""float64 numpy restatement of the baseline SELD features (the reference's dataset/feature_extraction.py) for the tests:
librosa.stft semantics (periodic Hann of win_len centred in the FFT frame, reflect padding, float64 evaluation stored as
complex64), power / IV in float32, GCC-PHAT's inverse FFT in float64 (the reference's numpy 1.19)."""
import numpy as np

PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def stft(y, n_fft, hop, win_len):
    """(n_fft//2 + 1, T) complex64 of one channel"""
    w = np.zeros(n_fft)
    n = np.arange(win_len)
    lp = (n_fft - win_len) // 2
    w[lp:lp + win_len] = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_len)
    yp = np.pad(np.asarray(y, np.float64), n_fft // 2, mode='reflect')
    T = 1 + len(y) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.fft.rfft(yp[idx] * w, axis=1).T.astype(np.complex64)


def mel_matrix(fs, n_fft, n_mels, fmin, fmax):
    """librosa 0.8.0 filters.mel (Slaney scale and norm), float32"""
    f_sp, lo_hz = 200.0 / 3, 1000.0
    lo_mel, step = lo_hz / f_sp, np.log(6.4) / 27.0

    def to_mel(f):
        return lo_mel + np.log(f / lo_hz) / step if f >= lo_hz else f / f_sp

    def to_hz(m):
        m = np.asarray(m, np.float64)
        return np.where(m >= lo_mel, lo_hz * np.exp(step * (m - lo_mel)), f_sp * m)
    fft_f = np.linspace(0, fs / 2.0, 1 + n_fft // 2)
    mel_f = to_hz(np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2))
    W = np.zeros((n_mels, 1 + n_fft // 2), np.float32)
    for i in range(n_mels):
        down = (fft_f - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        up = (mel_f[i + 2] - fft_f) / (mel_f[i + 2] - mel_f[i + 1])
        W[i] = np.maximum(0, np.minimum(down, up))
    W *= (2.0 / (mel_f[2:] - mel_f[:-2]))[:, None]
    return W


def lin_matrix(n_fft, compress=True):
    F = (200 if n_fft == 512 else 100) if compress else n_fft // 2
    ident = (192 if n_fft == 512 else 96) if compress else n_fft // 2
    W = np.zeros((F, n_fft // 2 + 1), np.float32)
    for i in range(ident):
        W[i, i + 1] = 1.0
    for i in range(ident, F):
        a = ident + 1 + (i - ident) * 8
        W[i, a:a + (8 if i < F - 1 else 7)] = 0.125
    return W


def db(p):
    return (10.0 * np.log10(np.maximum(np.float32(1e-10), p))).astype(np.float32)


def gcc(Xm, Xn, L, f64):
    """kept lags (T, L) of irfft(exp(i angle(Xm conj(Xn)))) in float64"""
    R = Xm.astype(np.complex128) * np.conj(Xn.astype(np.complex128)) if f64 else Xm * np.conj(Xn)
    ph = np.exp(1j * np.angle(R).astype(np.float64))
    cc = np.fft.irfft(ph, axis=0).T
    return np.concatenate((cc[:, -(L // 2 + L % 2):], cc[:, :L // 2]), axis=1)


def extract(feature_type, audio, fs=24000, n_fft=512, hop=300, win_len=None, n_mels=128, fmin=50, fmax=12000, compress=True):
    """(C, T, F) float32 of one (4, N) clip"""
    win_len = win_len or n_fft
    lin = feature_type.startswith('lin')
    W = lin_matrix(n_fft, compress) if lin else mel_matrix(fs, n_fft, n_mels, fmin, fmax)
    X = [stft(audio[c], n_fft, hop, win_len) for c in range(4)]
    rows = [db((W @ (np.abs(x) ** 2)).T) for x in X]
    if feature_type.endswith('iv'):
        iv = [np.real(np.conj(X[0]) * X[j]) for j in (1, 2, 3)]
        nrm = np.sqrt(iv[0] ** 2 + iv[1] ** 2 + iv[2] ** 2) + np.float32(1e-8)
        rows += [(W @ (v / nrm)).T for v in iv]
    elif feature_type.endswith('gcc'):
        n2 = 2 * n_fft
        X2 = [stft(audio[c], n2, hop, win_len) for c in range(4)]
        rows += [gcc(X2[m], X2[n], W.shape[0], not lin) for n, m in PAIRS]
    return np.stack(rows).astype(np.float32)
