"""Settings and built clips of the off-default tests of the baseline feature kernels (test_baseline_off_default_cpu.py fixes the
constants from the float64 restatement alone, test_baseline_off_default_gpu.py holds the kernels to it).  Plain data and small
seeded builders."""
import numpy as np

MEL = ('melspec', 'melspeciv', 'melspecgcc')
LIN = ('linspeciv', 'linspecgcc')
ALL = MEL + LIN

# (name, (fs, n_fft, hop, win_len, n_mels, fmin, fmax, compress), feature types).  The lin types ignore the mel fields, the mel
# types ignore compress.  fmax None: fs / 2.
SETTINGS = [
    # ---- n_fft 512
    ('512_hop240', (24000, 512, 240, 512, 128, 50, 12000, True), ALL),
    ('512_hop160', (24000, 512, 160, 512, 128, 50, 12000, True), ('melspeciv', 'linspecgcc')),
    ('512_hop600', (24000, 512, 600, 512, 128, 50, 12000, True), ('melspec', 'melspecgcc', 'linspeciv')),      # hop > n_fft
    ('512_win511', (24000, 512, 300, 511, 128, 50, 12000, True), ALL),                                          # odd window
    ('512_win400', (24000, 512, 300, 400, 128, 50, 12000, True), ('melspecgcc', 'linspecgcc')),                 # the second window
    ('512_win128', (24000, 512, 300, 128, 128, 50, 12000, True), ('melspeciv', 'linspecgcc')),
    ('512_mels40', (24000, 512, 300, 512, 40, 50, 12000, True), ('melspec', 'melspecgcc')),
    ('512_mels96', (24000, 512, 300, 512, 96, 50, 12000, True), ('melspeciv',)),
    ('512_mels127', (24000, 512, 300, 512, 127, 50, 12000, True), ('melspeciv', 'melspecgcc')),                 # odd F
    ('512_full', (24000, 512, 300, 512, 128, 50, 12000, False), LIN),                                           # F = 256
    # ---- n_fft 256
    ('256_mels63', (24000, 256, 150, 256, 63, 50, 12000, True), ('melspeciv', 'melspecgcc')),                   # odd F
    ('256_mels129', (24000, 256, 150, 256, 129, 50, 12000, True), MEL),                                         # odd F, rows of one bin or none
    ('256_mels256', (24000, 256, 150, 256, 256, 50, 12000, True), ('melspeciv', 'melspecgcc')),                 # many empty rows
    ('256_win200', (24000, 256, 100, 200, 64, 50, 12000, True), ALL),
    ('256_full', (24000, 256, 150, 256, 64, 50, 12000, False), LIN),                                            # F = 128
    ('256_comp', (24000, 256, 150, 256, 64, 50, 12000, True), LIN),                                             # F = 100
    # ---- other rates and band edges
    ('16k_fmin0', (16000, 512, 200, 512, 64, 0, None, True), MEL),
    ('48k_100_20k', (48000, 512, 480, 512, 96, 100, 20000, True), ('melspeciv', 'melspecgcc')),
    ('16k_nyquist', (16000, 256, 128, 256, 64, 50, 8000, True), ('melspec', 'melspecgcc')),                     # fmax == fs / 2
]

# one setting per kernel instantiation (n_fft x spec / IV / GCC)
INSTANTIATIONS = [('512_hop240', 'melspec'), ('512_win511', 'linspeciv'), ('512_mels127', 'melspecgcc'),
                  ('256_mels129', 'melspec'), ('256_win200', 'melspeciv'), ('256_full', 'linspecgcc')]

DELAYS = (0, 3, 7, 12)                      # 'delayed': channel c is the source delayed by DELAYS[c] samples
FAMILIES = ('delayed', 'silent1', 'impulse', 'silent_middle', 'tiny', 'full_scale', 'dc', 'lowpass', 'silent0')
BATCHES = (FAMILIES[0:3], FAMILIES[3:6], FAMILIES[6:9])
MAX_SAMPLES = 8000


def setting(name):
    return next(s for s in SETTINGS if s[0] == name)


def keywords(cfg):
    """the setting as BaselineExtractor's keywords"""
    fs, n_fft, hop, win_len, n_mels, fmin, fmax, compress = cfg
    return dict(fs=fs, n_fft=n_fft, hop_len=hop, win_len=win_len, n_mels=n_mels, fmin=fmin, fmax=fmax, is_compressed_freq=compress)


def n_freq(cfg, feature_type):
    _, n_fft, _, _, n_mels, _, _, compress = cfg
    if feature_type in MEL:
        return n_mels
    return ((200 if n_fft == 512 else 100) if compress else n_fft // 2)


def pad_of(cfg, feature_type):
    """samples the STFT reflects at each clip end: n_fft / 2, and n_fft for the GCC types' second transform"""
    return cfg[1] if feature_type.endswith('gcc') else cfg[1] // 2


def lengths(cfg, feature_type):
    """the shortest clip the host accepts, pad + hop, a multiple of hop (last frame centred on the clip's end), one less, ~12 frames"""
    pad, hop = pad_of(cfg, feature_type), cfg[2]
    k = pad // hop + 2
    out = [pad + 1, pad + hop, k * hop, (k + 1) * hop - 1, 12 * hop + hop // 3]
    assert max(out) <= MAX_SAMPLES and min(out) > pad
    return out


def _noise(rng, n):
    """4 channels: one white source at the known delays + 10 % independent noise per channel"""
    D = max(DELAYS)
    src = rng.randn(n + D)
    return np.stack([src[D - d:D - d + n] for d in DELAYS]) + 0.1 * rng.randn(4, n)


def clip(family, n, pad, seed=0):
    """(4, n) float32 of one family; `pad` places the impulses"""
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + seed)
    if family == 'delayed':                      # exactly delayed copies: the GCC peak lag of pair (n, m) is d_m - d_n
        D = max(DELAYS)
        src = 0.25 * rng.randn(n + D)
        y = np.stack([src[D - d:D - d + n] for d in DELAYS])
    elif family in ('silent1', 'silent0'):
        y = 0.25 * _noise(rng, n)
        y[int(family[-1])] = 0.0
    elif family == 'impulse':                    # only the reflection carries these into the first and last frames' far halves
        # (over -60 dB of noise: frame 0 is symmetric about its centre, so an impulse and its mirror image alone have an exactly
        # real cosine spectrum, and at its zero crossings a float64 FFT leaves round-off whose phase nothing pins)
        y = 1e-3 * rng.randn(4, n)
        for c in range(4):
            y[c, min(1 + 5 * c, pad - 1)] = 1.0
            y[c, max(n - 2 - 3 * c, n - pad)] = 1.0
    elif family == 'silent_middle':
        y = 0.25 * _noise(rng, n)
        y[:, n // 3:2 * n // 3] = 0.0
    elif family == 'tiny':                       # power under the 1e-10 clamp
        y = 1e-6 * _noise(rng, n)
    elif family == 'full_scale':
        y = np.where(_noise(rng, n) >= 0, 1.0, -1.0)
    elif family == 'dc':
        y = 0.5 + 0.1 * _noise(rng, n)
    elif family == 'lowpass':                    # bins above fs / 8 hold the float32 rounding of the samples only
        S = np.fft.rfft(0.25 * _noise(rng, n), axis=1)
        S[:, S.shape[1] // 4:] = 0.0
        y = np.fft.irfft(S, n, axis=1)
    else:
        raise KeyError(family)
    return np.ascontiguousarray(y, np.float32)


def entries():
    """every (setting name, cfg, feature type, n_samples, families of the batch) the GPU module extracts and compares: each length
    takes one batch of 3 families, rotated so that every family meets every kind of length across the settings"""
    for si, (name, cfg, types) in enumerate(SETTINGS):
        for ti, ft in enumerate(types):
            for li, n in enumerate(lengths(cfg, ft)):
                yield name, cfg, ft, n, BATCHES[(si + ti + li) % 3]
