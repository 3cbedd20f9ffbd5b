"""Spatially diffuse ambient noise for the rendered scenes.  The reference has no such code; the definition is
this project's.  A diffuse field is D uncorrelated plane-wave noises from the D directions of a Fibonacci lattice, each reaching the
array through the direct-path response a point source gets (`mix`), followed by one colouring filter:

    m[c][t] = sum_d sum_k mix[d][c][k] white(seed_b, d, t - k)          float32, fmaf chain, d outer, k inner, ascending
    y[c][n] = sum_j colour[j] m[c][n - j]                               float32, fmaf chain, j ascending
    out[b][c][n] = fmaf(scale_b, y[c][n], in[b][c][n])                  (in absent: scale_b y[c][n])

white(seed, d, n) is a counter hash (white_fields below states it), defined for n >= -1024, so the noise has no onset at sample 0.  The
sums run in salsa_amd/csrc/scene_diffuse.hip (include/salsa_hip.h: salsa_scene_diffuse); SALSA_HIP_SCENE=0 or device='cpu' sends them to
a composed torch evaluation of the same definition (the hash in int64 tensor arithmetic, conv1d).  The expected power per channel at
scale 1 is known exactly, P_c = sum_d ||mix[d][c] * colour||^2, so the scale for a level or an SNR is computed, never measured."""
import ctypes as C

import numpy as np

from . import _lib
from . import scenes as _sc
from .scenes import FS, MIC_DIRECTIONS, MIC_RADIUS, SINC_HALF, SOUND_SPEED

MAX_DIRECTIONS, MAX_MIX_TAPS, MAX_COLOUR_TAPS = 256, 128, 513        # the launcher's limits (include/salsa_hip.h)
COLOUR_TAPS, COLOUR_NFFT = 513, 8192                                # a preset's taps; the frequency grid its magnitude is sampled on
WHITE_LEAD = 1024                                                   # white(seed, d, n) is defined for n >= -WHITE_LEAD
WHITE_SCALE = float(np.float32(np.sqrt(3.0 / (65536.0 ** 2 - 1.0))))   # Irwin-Hall of four 16-bit fields to variance 1
_GOLDEN, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
TORCH_CHUNK = 1 << 16                                               # samples per step of the composed torch path


def fibonacci_sphere(n):
    """n unit vectors (x, y, z) float64 spread evenly over the sphere: z_i = 1 - (2 i + 1) / n, azimuth i times the golden angle"""
    i = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


def colour_filter(colour, fs=FS, taps=COLOUR_TAPS):
    """The colouring filter, float64 (Lg,), Lg odd: a linear-phase FIR by frequency sampling (COLOUR_NFFT bins) under a Hann window,
    normalised to unit energy.  'white': the unit impulse (Lg = 1); 'pink': power 1 / f above 50 Hz, flat below; 'room': power falling
    5 dB per octave above 125 Hz, flat below, a plain stand-in for ventilation noise; or a pair (freqs Hz ascending, magnitudes >= 0),
    interpolated linearly."""
    if isinstance(colour, str) and colour == 'white':
        return np.ones(1, np.float64)
    taps = int(taps)
    if not (1 <= taps <= MAX_COLOUR_TAPS and taps % 2 == 1):
        raise ValueError('a colour filter has an odd number of 1 .. %d taps' % MAX_COLOUR_TAPS)
    f = np.fft.rfftfreq(COLOUR_NFFT, 1.0 / fs)
    if isinstance(colour, str):
        if colour == 'pink':
            mag = (np.maximum(f, 50.0) / 50.0) ** -0.5
        elif colour == 'room':
            mag = 10.0 ** (-5.0 / 20.0 * np.log2(np.maximum(f, 125.0) / 125.0))
        else:
            raise ValueError("colour is 'white', 'pink', 'room' or (freqs, magnitudes)")
    else:
        freqs, mags = (np.asarray(a, np.float64).reshape(-1) for a in colour)
        if len(freqs) != len(mags) or len(freqs) < 1 or np.any(np.diff(freqs) <= 0) or np.any(mags < 0) or not np.any(mags > 0):
            raise ValueError('(freqs, magnitudes): ascending frequencies, magnitudes >= 0 and not all 0')
        mag = np.interp(f, freqs, mags)
    h0 = np.fft.irfft(mag, COLOUR_NFFT)
    h = h0[(np.arange(taps) - (taps - 1) // 2) % COLOUR_NFFT] * np.hanning(taps + 2)[1:-1]
    h = 0.5 * (h + h[::-1])                                                   # exactly symmetric: the transform's rounding is not
    return h / np.sqrt(np.sum(h * h))


class DiffuseField:
    """.directions float64 (D, 3) unit vectors (x, y, z); .mix float32 (D, 4, La), built in float64 and rounded once; .colour float64
    (Lg,) of unit energy and .colour32, its float32 rounding, which is what is rendered; .channel_power float64 (4,), the expected mean
    square per channel at scale 1, of the float32 filters as they are.
    foa: La = 1, the gains (1, u_y, u_z, u_x).  mic, baffle='open': the Hann-windowed sinc of half width SINC_HALF at each capsule's
    advance p_m . u fs / c, around the common lead SINC_HALF + ceil(R fs / c) (La = 2 lead + 1 = 39 at 24 kHz: every capsule's whole
    support).  mic, baffle='rigid': rooms.SphereTable.weights at the capsule's angle to the direction, the far-field model of
    salsa_room_rirs_sphere (La = lead + trail + 1 = 80)."""

    def __init__(self, audio_format, baffle='open', n_directions=64, colour='room', fs=FS):
        from . import rooms
        if audio_format not in _lib.FORMAT:
            raise ValueError('audio_format must be foa or mic')
        rigid = rooms._check_baffle(audio_format, baffle)
        D = int(n_directions)
        if not 1 <= D <= MAX_DIRECTIONS:
            raise ValueError('1 .. %d directions' % MAX_DIRECTIONS)
        self.audio_format, self.baffle, self.fs = audio_format, baffle, float(fs)
        u = self.directions = fibonacci_sphere(D)
        if audio_format == 'foa':
            mix = np.stack([np.ones(D), u[:, 1], u[:, 2], u[:, 0]], axis=1)[:, :, None]
        elif rigid:
            st = rooms.sphere_table(MIC_RADIUS, fs, SOUND_SPEED)
            theta = np.arccos(np.clip(u @ rooms._capsule_units().T, -1.0, 1.0))                       # (D, 4)
            mix = st.weights(theta[:, :, None], np.arange(st.lead + st.trail + 1, dtype=np.float64)[None, None, :] - st.lead)
        else:
            lead = SINC_HALF + int(np.ceil(MIC_RADIUS * fs / SOUND_SPEED))
            centre = lead - (u @ (MIC_RADIUS * rooms._capsule_units()).T) * fs / SOUND_SPEED          # an advance moves the peak earlier
            mix = rooms._windowed_sinc(np.arange(2 * lead + 1, dtype=np.float64)[None, None, :] - centre[:, :, None])
        self.mix = np.ascontiguousarray(mix, np.float32)
        self.colour = colour_filter(colour, fs)
        self.colour32 = np.ascontiguousarray(self.colour, np.float32)
        if self.mix.shape[2] > MAX_MIX_TAPS:
            raise ValueError('the array response has %d taps at fs = %g, more than %d' % (self.mix.shape[2], fs, MAX_MIX_TAPS))
        g = self.colour32.astype(np.float64)
        self.channel_power = np.array([sum(np.sum(np.convolve(self.mix[d, c].astype(np.float64), g) ** 2) for d in range(D))
                                       for c in range(4)], np.float64)
        self._dev = {}

    n_directions = property(lambda self: self.mix.shape[0])
    mix_taps = property(lambda self: self.mix.shape[2])
    colour_taps = property(lambda self: len(self.colour32))

    def response(self, freqs):
        """F[f, d, c] = sum_k mix[d][c][k] exp(-2 pi i f k / fs), complex128"""
        f = np.asarray(freqs, np.float64).reshape(-1)
        e = np.exp(-2j * np.pi * f[:, None] * np.arange(self.mix_taps)[None, :] / self.fs)
        return np.einsum('dck,fk->fdc', self.mix.astype(np.float64), e)

    def coherence(self, freqs):
        """The expected coherence between the channels that the filters imply, complex128 (len(freqs), 4, 4): sum_d F_di conj(F_dj)
        over the square root of the two channels' powers.  The colour is common to all channels and cancels."""
        F = self.response(freqs)
        S = np.einsum('fdi,fdj->fij', F, np.conj(F))
        p = np.real(np.einsum('fii->fi', S))
        return S / np.sqrt(p[:, :, None] * p[:, None, :])

    def scale_for(self, level_db):
        """the scale at which the mean square averaged over the four channels is expected to be 10^(level_db / 10), float64"""
        return np.sqrt(10.0 ** (np.asarray(level_db, np.float64) / 10.0) / self.channel_power.mean())

    def on(self, device):
        """(mix, colour32) as tensors on `device`, uploaded once"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.mix).to(device), torch.from_numpy(self.colour32).to(device))
        return self._dev[key]


# ---- white(seed, d, n) in int64 tensor arithmetic (two's complement wraps as uint64 does) --------------------------------------------------
def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _mix64(z):
    z = z ^ ((z >> 30) & ((1 << 34) - 1))                                  # a logical shift: the sign's copies are masked off
    z = z * _s64(_M1)
    z = z ^ ((z >> 27) & ((1 << 37) - 1))
    z = z * _s64(_M2)
    return z ^ ((z >> 31) & ((1 << 33) - 1))


def white_fields(seeds, d, n):
    """The four 16-bit fields of the hash, int64 tensors (B, D, T, 4), for seeds (B,), directions d (D,), samples n (T,) >= -WHITE_LEAD,
    all int64 tensors (a seed is the uint64's bits):
        mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31          (mod 2^64)
        h = mix64(mix64(seed + G) + ((d << 48) | (n + 1024)) G),  G = 0x9E3779B97F4A7C15;   u_i = (h >> 16 i) & 0xFFFF"""
    import torch
    key = _mix64(seeds + _s64(_GOLDEN))
    idx = (d[:, None] << 48) | (n[None, :] + WHITE_LEAD)
    h = _mix64(key[:, None, None] + idx[None] * _s64(_GOLDEN))
    return torch.stack([(h >> s) & 0xFFFF for s in (0, 16, 32, 48)], dim=-1)


def white(seeds, d, n):
    """white(seed, d, n) = float32(u_0 + u_1 + u_2 + u_3 - 131070) WHITE_SCALE, float32 (B, D, T): mean 0, variance 1"""
    import torch
    return (white_fields(seeds, d, n).sum(dim=-1) - 131070).to(torch.float32) * WHITE_SCALE


def _diffuse_torch(field, seeds, scales, inp, out):
    """the definition composed from torch calls, clip by clip and TORCH_CHUNK samples at a time"""
    import torch
    import torch.nn.functional as F
    dev = out.device
    mix, colour = field.on(dev)
    D, La, Lg = field.n_directions, field.mix_taps, field.colour_taps
    B, _, N = out.shape
    w_mix = mix.permute(1, 0, 2).flip(-1).contiguous()                       # conv1d correlates: (4, D, La), taps reversed
    w_col = colour.flip(0).view(1, 1, Lg)
    dirs = torch.arange(D, dtype=torch.int64, device=dev)
    for b in range(B):
        live = scales[b] != 0
        for lo in range(0, N, TORCH_CHUNK):
            hi = min(N, lo + TORCH_CHUNK)
            n = torch.arange(lo - (Lg - 1) - (La - 1), hi, dtype=torch.int64, device=dev)
            m = F.conv1d(white(seeds[b:b + 1], dirs, n), w_mix)              # (1, 4, hi - lo + Lg - 1)
            y = F.conv1d(m.view(4, 1, -1), w_col).view(4, hi - lo)
            base = inp[b, :, lo:hi] if inp is not None else torch.zeros_like(y)
            out[b, :, lo:hi] = torch.where(live, base + scales[b] * y, base)
    return out


def _diffuse_hip(field, seeds, scales, inp, out):
    import torch
    L = _lib.load()
    dev = out.device
    mix, colour = field.on(dev)
    D, La, Lg = field.n_directions, field.mix_taps, field.colour_taps
    B, Cn, N = out.shape
    if not L.salsa_scene_diffuse_supported(Cn, D, La, Lg):
        raise ValueError('salsa_scene_diffuse does not take %d channels, %d directions, %d mix taps, %d colour taps' % (Cn, D, La, Lg))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(dev):
        rc = L.salsa_scene_diffuse(ptr(mix), D, Cn, La, ptr(colour), Lg, ptr(seeds), ptr(scales), ptr(inp), ptr(out), B, N,
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc:
        raise RuntimeError('salsa_scene_diffuse failed (%d): %s' % (rc, _lib.last_error()))
    return out


def _seeds_on(seeds, n_clips, device):
    """None: 0, 1, ..; an integer seed0: seed0 + clip index (mod 2^64); else one seed per clip.  -> int64 tensor of the uint64s' bits"""
    import torch
    if torch.is_tensor(seeds):
        t = seeds.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    else:
        if seeds is None or np.ndim(seeds) == 0:
            seeds = [(int(0 if seeds is None else seeds) + b) % (1 << 64) for b in range(n_clips)]
        t = torch.from_numpy(np.array([int(s) % (1 << 64) for s in seeds], np.uint64).view(np.int64)).to(device)
    if t.numel() != n_clips:
        raise ValueError('one seed per clip')
    return t


def _run(field, seeds, scales, inp, out):
    import torch
    B, Cn, N = out.shape
    if Cn != 4 or B < 1 or N < 1:
        raise ValueError('diffuse noise is rendered into (B, 4, N) with B, N >= 1')
    for t in (inp, out):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, Cn, N) and t.device == out.device):
            raise ValueError('contiguous float32 (%d, %d, %d) tensors on one device expected' % (B, Cn, N))
    seeds = _seeds_on(seeds, B, out.device)
    scales = scales.to(device=out.device, dtype=torch.float32).expand(B).contiguous()
    if out.is_cuda and _sc.HIP_SCENE:
        return _diffuse_hip(field, seeds, scales, inp, out)
    return _diffuse_torch(field, seeds, scales, inp, out)


def diffuse_noise(field, n_clips, n_samples, level_db=-60.0, seeds=None, device=None):
    """-> float32 (n_clips, 4, n_samples) on `device` (default 'cuda'): the field's noise alone.  level_db: the expected mean square
    averaged over the four channels, in dB re full scale (a scalar or one per clip).  seeds: None (clip b gets b), an integer seed0 (clip
    b gets seed0 + b) or one seed per clip."""
    import torch
    device = torch.device('cuda' if device is None else device)
    out = torch.empty((int(n_clips), 4, int(n_samples)), dtype=torch.float32, device=device)
    scales = torch.as_tensor(field.scale_for(level_db), dtype=torch.float32).reshape(-1)
    return _run(field, seeds, scales, None, out)


def add_diffuse(audio, field, snr_db=None, level_db=None, seeds=None, out=None):
    """Adds the field's noise to audio (B, 4, N) float32 and returns the sum: in `out`, or in `audio` itself when out is None.  Exactly
    one of snr_db (per clip, against the clip's mean square over all channels and samples; a silent clip gets scale 0 and keeps its
    bits) and level_db (as for diffuse_noise) is given, a scalar or one per clip.  The scales are computed on audio's device with torch
    operators and stay there: nothing is synchronised."""
    import torch
    if (snr_db is None) == (level_db is None):
        raise ValueError('exactly one of snr_db and level_db')
    if audio.dim() != 3:
        raise ValueError('audio is (B, 4, N)')
    B = audio.shape[0]
    if level_db is not None:
        scales = torch.as_tensor(field.scale_for(level_db), dtype=torch.float32).reshape(-1)
    else:
        power = torch.linalg.vector_norm(audio.reshape(B, -1), dim=1, dtype=torch.float64) ** 2 / (audio.shape[1] * audio.shape[2])
        ratio = 10.0 ** (torch.as_tensor(snr_db, dtype=torch.float64, device=audio.device).reshape(-1) / 10.0)
        scales = torch.sqrt(power / (ratio * float(field.channel_power.mean()))).to(torch.float32)
    return _run(field, seeds, scales, audio, audio if out is None else out)
