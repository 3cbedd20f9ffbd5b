"""Labelled SELD scenes rendered on the GPU: isolated events convolved with multichannel room impulse
responses of known directions, the DCASE data generator's recipe, so that audio exists whose labels mean something.  The reference
has no such code; the definition is this project's.

A scene is the item list of one clip; item i is (event e_i, rir r_i, onset o_i, gain g_i, class c_i, track t_i).

    audio[b, c, n] = ambient[b, c, n] + sum_i g_i (h[r_i, c, :] * s[e_i])[n - o_i]          0 <= n < N

with `*` the full linear convolution.  Item i is active in label frame f iff its DRY extent [o_i, o_i + len) meets
[hop f, hop (f + 1)), hop = fs / label_rate; its row is (f, c_i, t_i, azimuth[r_i], elevation[r_i]) in integer degrees, a DCASE
metadata CSV's row.  The convolutions run in salsa_amd/csrc/scene_render.hip (include/salsa_hip.h: salsa_scene_*); SALSA_HIP_SCENE=0
sends render_scenes to a composed torch.fft evaluation of the same definition, for A/B runs.

Moving sources: an item may carry a trajectory of responses r_{i,0} .. r_{i,K-1}, node k at dry time k S (S =
Scenes.traj_step samples, K = ceil((len - 1) / S) + 1).  With the windows w_k(n) = max(0, 1 - |n - k S| / S), which sum to one on
[0, len), the item contributes g_i sum_k (h[r_{i,k}, c, :] * (w_k . s_i))[n - o_i]: the input is cross-faded linearly from response to
response.  It is active in the frames its dry extent meets, as before; frame f carries the direction of the node nearest the frame's
centre, a tie going to the later one.  Scenes with a trajectory are rendered by salsa_scene_render_moving from a segment table."""
import ctypes as C
import io
import os

import numpy as np

from . import _lib

HIP_SCENE = os.environ.get('SALSA_HIP_SCENE', '1') != '0'   # 0: render_scenes composes torch.fft calls, for A/B runs and bisecting
FS = 24000
MAX_CHANNELS, MAX_RIR_LEN, MAX_ITEMS_PER_CLIP = 16, 16384, 256          # the launchers' limits (include/salsa_hip.h)
MAX_SEGMENTS_PER_CLIP, MIN_TRAJ_STEP, MAX_TRAJ_STEP = 65536, 240, 1 << 24  # salsa_scene_render_moving's
PART = 512                                                               # the renderer's partition, samples
SOUND_SPEED = 343.0
MIC_RADIUS = 0.042
MIC_DIRECTIONS = ((45, 35), (-45, -35), (135, -35), (-135, 35))          # the TNSSE tetrahedron (azimuth, elevation), degrees
SINC_HALF = 16                                                           # half width of the Hann-windowed sinc, samples


def _unit(az_deg, el_deg):
    az, el = np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(np.asarray(el_deg, np.float64))
    return np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=-1)          # (x, y, z)


class RirBank:
    """rirs float32 (R, C, L) with the integer-degree direction of each response.  Measured SRIRs (TAU-SRIR, ...) enter here as plain
    arrays; make_rir_bank builds synthetic ones.  The partition spectra are made once per device, on first use there."""

    def __init__(self, rirs, azimuth, elevation, audio_format='foa'):
        rirs = np.ascontiguousarray(rirs, np.float32)
        if rirs.ndim != 3 or not (1 <= rirs.shape[1] <= MAX_CHANNELS and 1 <= rirs.shape[2] <= MAX_RIR_LEN) or rirs.shape[0] < 1:
            raise ValueError('rirs must be (R, C, L) with 1 <= C <= %d and 1 <= L <= %d, got %s' % (MAX_CHANNELS, MAX_RIR_LEN, rirs.shape))
        if audio_format not in _lib.FORMAT:
            raise ValueError('audio_format must be foa or mic')
        self.rirs, self.audio_format = rirs, audio_format
        self.azimuth, self.elevation = np.asarray(azimuth, np.int64).reshape(-1), np.asarray(elevation, np.int64).reshape(-1)
        if len(self.azimuth) != rirs.shape[0] or len(self.elevation) != rirs.shape[0]:
            raise ValueError('one azimuth and one elevation per response')
        self._spectra = {}

    n_rirs = property(lambda self: self.rirs.shape[0])
    n_channels = property(lambda self: self.rirs.shape[1])
    length = property(lambda self: self.rirs.shape[2])

    def rirs_on(self, device):
        import torch
        return torch.from_numpy(self.rirs).to(device)

    def nearest(self, azimuth, elevation):
        """index of the response at the least great-circle angle from (azimuth, elevation) in degrees; the lowest index on a tie"""
        cosine = np.clip(_unit(self.azimuth, self.elevation) @ _unit(azimuth, elevation).T, -1.0, 1.0)    # (R,) or (R, n) for arrays
        idx = np.argmin(np.arccos(cosine), axis=0)
        return int(idx) if np.ndim(idx) == 0 else idx.astype(np.int64)

    @staticmethod
    def device_key(device):
        import torch
        device = torch.device(device)
        return (device.type, device.index if device.index is not None else torch.cuda.current_device())

    def spectra(self, device):
        key = self.device_key(device)
        if key not in self._spectra:
            self._spectra[key] = rir_spectra(self.rirs_on(device))            # once per bank and device
        return self._spectra[key]

    def acoustics(self, device=None, **kw):
        """rooms.rir_acoustics of the bank's responses: decay times, DRR, C50 per (response, channel)"""
        from . import rooms
        return rooms.rir_acoustics(self.rirs, device=device, **kw)


def rir_spectra(d_rirs):
    """The partition spectra (salsa_scene_rir_spectra) of contiguous float32 CUDA responses (R, C, L), on their device.  A bank whose
    responses were generated on a device (rooms.room_rir_bank) gets its spectra from here before the download."""
    import torch
    L = _lib.load()
    R, Cn, Ln = d_rirs.shape
    device = d_rirs.device
    n = L.salsa_scene_rir_spectra_bytes(R, Cn, Ln)
    spec = torch.empty(n // 4, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        rc = L.salsa_scene_rir_spectra(C.c_void_p(d_rirs.data_ptr()), R, Cn, Ln, C.c_void_p(spec.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc:
        raise RuntimeError('salsa_scene_rir_spectra failed (%d): %s' % (rc, _lib.last_error()))
    torch.cuda.current_stream(device).synchronize()                           # d_rirs may go now
    return spec


def _rigid_direct(d, length, fs):
    """make_rir_bank('mic', baffle='rigid'): the free-field direct path on the rigid sphere, float64 (R, 4, length) and the tail's start"""
    from . import rooms
    st = rooms.sphere_table(MIC_RADIUS, fs, SOUND_SPEED)
    t0 = st.lead + st.trail
    if length < t0 + 1:
        raise ValueError('a rigid mic response needs at least %d taps' % (t0 + 1))
    theta = np.arccos(np.clip(d @ _unit([m[0] for m in MIC_DIRECTIONS], [m[1] for m in MIC_DIRECTIONS]).T, -1.0, 1.0))      # (R, 4)
    h = np.zeros((len(d), 4, length), np.float64)
    h[:, :, :t0 + 1] = st.weights(theta[:, :, None], np.arange(t0 + 1, dtype=np.float64)[None, None, :] - st.lead)
    return h, t0


def make_rir_bank(audio_format, directions, length, rt60=None, drr_db=6.0, seed=0, fs=FS, baffle='open'):
    """Synthetic responses for `directions` = [(azimuth, elevation), ...] in integer degrees, float64 -> float32.
    foa: channels W, Y, Z, X (the order the reference's FOA transform documents); the direct path is ONE tap (index 0) with the gains
    (1, sin az cos el, sin el, cos az cos el).  mic: the TNSSE tetrahedron, a plane wave from the direction; microphone m hears it
    p_m . d / c seconds early, a Hann-windowed-sinc fractional delay around tap SINC_HALF (length >= 2 SINC_HALF + 1).
    rt60 (seconds): adds a diffuse tail after the direct path, Gaussian noise independent per channel decaying by 60 dB per rt60, whose
    energy per channel is the first channel's direct energy / 10^(drr_db / 10); RandomState(seed) stream, frozen by numpy.
    baffle='rigid' (mic only): the capsules sit on a rigid sphere of MIC_RADIUS; the direct path is rooms.
    SphereTable.weights at each capsule's angle from the direction, the array centre at tap `lead`, the tail after tap lead + trail."""
    directions = np.asarray(directions, np.int64).reshape(-1, 2)
    d = _unit(directions[:, 0], directions[:, 1])                             # (R, 3)
    R = len(d)
    h = np.zeros((R, 4, length), np.float64)
    if baffle not in ('open', 'rigid'):
        raise ValueError("baffle is 'open' or 'rigid'")
    if baffle == 'rigid':
        if audio_format != 'mic':
            raise ValueError("baffle='rigid' is the mic format's")
        h, t0 = _rigid_direct(d, length, fs)
    elif audio_format == 'foa':
        h[:, 0, 0], h[:, 1, 0], h[:, 2, 0], h[:, 3, 0] = 1.0, d[:, 1], d[:, 2], d[:, 0]
        t0 = 0
    elif audio_format == 'mic':
        if length < 2 * SINC_HALF + 1:
            raise ValueError('a mic response needs at least %d taps' % (2 * SINC_HALF + 1))
        mics = MIC_RADIUS * _unit([m[0] for m in MIC_DIRECTIONS], [m[1] for m in MIC_DIRECTIONS])     # (4, 3)
        centre = SINC_HALF - (d @ mics.T) * fs / SOUND_SPEED                  # (R, 4): an advance moves the peak earlier
        n = np.arange(2 * SINC_HALF + 1, dtype=np.float64)
        x = n[None, None, :] - centre[:, :, None]
        win = np.where(np.abs(x) <= SINC_HALF, 0.5 * (1.0 + np.cos(np.pi * x / SINC_HALF)), 0.0)
        h[:, :, :2 * SINC_HALF + 1] = np.sinc(x) * win
        t0 = 2 * SINC_HALF
    else:
        raise ValueError('audio_format must be foa or mic')
    if rt60 is not None and length > t0 + 1:
        rng = np.random.RandomState(seed)
        t = np.arange(length - t0 - 1, dtype=np.float64)
        tail = rng.randn(R, 4, len(t)) * 10.0 ** (-3.0 * t / (rt60 * fs))
        direct = np.sum(h[:, :1] ** 2, axis=-1, keepdims=True)
        tail *= np.sqrt(direct / 10.0 ** (drr_db / 10.0) / np.sum(tail ** 2, axis=-1, keepdims=True))
        h[:, :, t0 + 1:] += tail
    return RirBank(h.astype(np.float32), directions[:, 0], directions[:, 1], audio_format)


class EventPool:
    """signals: 1-D float arrays (the dry, isolated events); classes: one sound class index each."""

    def __init__(self, signals, classes):
        self.signals = [np.ascontiguousarray(s, np.float32).reshape(-1) for s in signals]
        self.classes = np.asarray(classes, np.int64).reshape(-1)
        if not self.signals or len(self.signals) != len(self.classes) or min(len(s) for s in self.signals) < 1:
            raise ValueError('one class per signal, every signal at least one sample')
        self.lengths = np.array([len(s) for s in self.signals], np.int64)
        self.offset = np.concatenate(([0], np.cumsum(self.lengths))).astype(np.int64)
        self.flat = np.concatenate(self.signals)
        self.max_len = int(self.lengths.max())
        self._dev = {}

    def __len__(self):
        return len(self.signals)

    def on(self, device):
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.flat).to(device)
        return self._dev[key]


def synth_event_pool(n_classes=12, per_class=4, seed=0, fs=FS, min_s=0.4, max_s=2.0):
    """Class-distinct synthetic sounds, so that classes are learnable: class k owns a band around f_k (log-spaced 250 Hz .. 7 kHz) and one
    of three kinds by k % 3 -- band-limited noise, a harmonic stack on a class-specific fundamental, an up or down chirp across the band
    -- under a class-specific envelope (attack and decay times).  Instances differ in length, phase and noise.  RandomState streams
    (frozen by numpy), one per (seed, class, instance); peak-normalised to 0.5."""
    signals, classes = [], []
    fk = 250.0 * (7000.0 / 250.0) ** (np.arange(n_classes) / max(1, n_classes - 1))
    for k in range(n_classes):
        for j in range(per_class):
            rng = np.random.RandomState((seed * 1009 + k) * 1013 + j)
            n = int(rng.uniform(min_s, max_s) * fs)
            t = np.arange(n) / fs
            lo, hi = fk[k] / 1.25, fk[k] * 1.25
            if k % 3 == 0:                                                     # band-limited noise: a Gaussian band cut from white noise
                spec = np.fft.rfft(rng.randn(n))
                f = np.fft.rfftfreq(n, 1.0 / fs)
                x = np.fft.irfft(spec * np.exp(-0.5 * ((f - fk[k]) / (0.1 * fk[k])) ** 2), n)
            elif k % 3 == 1:                                                   # harmonic stack
                f0 = fk[k] / 3.0
                x = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h for h in range(1, 7) if f0 * h < 0.45 * fs)
                x = x + 0.02 * rng.randn(n)
            else:                                                              # chirp across the band, direction by class
                a, b = (lo, hi) if (k // 3) % 2 == 0 else (hi, lo)
                x = np.sin(2 * np.pi * (a * t + 0.5 * (b - a) * t * t / t[-1] if n > 1 else a * t) + rng.uniform(0, 2 * np.pi))
                x = x + 0.02 * rng.randn(n)
            attack, decay = 0.005 * (1 + k % 4), 0.05 * (1 + (k * 5) % 7)
            env = np.minimum(1.0, t / attack) * np.minimum(1.0, (t[-1] - t) / decay + 1e-3)
            if k % 2:
                env = env * (0.6 + 0.4 * np.cos(2 * np.pi * (2 + k) * t))      # a class-specific tremolo
            x = x * env
            signals.append((0.5 * x / max(np.abs(x).max(), 1e-12)).astype(np.float32))
            classes.append(k)
    return EventPool(signals, classes)


class Scenes:
    """The item tables of n_clips clips: clip b owns items clip_start[b] .. clip_start[b + 1] - 1.  Per item: event (index into the
    pool), rir (index into the bank), onset (samples), gain (linear), cls, track, length (of the dry event), azimuth and elevation
    (integer degrees of its response).  scenes[b] is clip b alone."""
    FIELDS = ('event', 'rir', 'onset', 'gain', 'cls', 'track', 'length', 'azimuth', 'elevation')
    TRAJ_FIELDS = ('traj_rir', 'traj_azimuth', 'traj_elevation')              # flat, one entry per trajectory node

    def __init__(self, n_samples, clip_start, traj_start=None, traj_rir=None, traj_azimuth=None, traj_elevation=None, traj_step=2400,
                 **items):
        """Trajectories (optional): item i owns nodes traj_start[i] .. traj_start[i + 1] - 1 of traj_rir (and of traj_azimuth /
        traj_elevation, the nodes' directions in integer degrees): none for a static item, exactly K = ceil((length - 1) / traj_step)
        + 1 for a moving one, whose rir / azimuth / elevation fields are those of node 0."""
        self.n_samples = int(n_samples)
        self.clip_start = np.asarray(clip_start, np.int32).reshape(-1)
        for f in self.FIELDS:
            setattr(self, f, np.asarray(items[f], np.float32 if f == 'gain' else np.int64).reshape(-1))
        n = len(self.event)
        if any(len(getattr(self, f)) != n for f in self.FIELDS) or len(self.clip_start) < 2 or self.clip_start[0] != 0 \
                or self.clip_start[-1] != n or np.any(np.diff(self.clip_start) < 0):
            raise ValueError('inconsistent scene tables')
        self.traj_step = int(traj_step)
        self.traj_start = np.zeros(n + 1, np.int64) if traj_start is None else np.asarray(traj_start, np.int64).reshape(-1)
        for f, v in zip(self.TRAJ_FIELDS, (traj_rir, traj_azimuth, traj_elevation)):
            setattr(self, f, np.asarray([] if v is None else v, np.int64).reshape(-1))
        if len(self.traj_start) != n + 1 or self.traj_start[0] != 0 or self.traj_start[-1] != len(self.traj_rir) \
                or any(len(getattr(self, f)) != len(self.traj_rir) for f in self.TRAJ_FIELDS):
            raise ValueError('inconsistent trajectory tables')
        nodes = np.diff(self.traj_start)
        if np.any(nodes < 0):
            raise ValueError('inconsistent trajectory tables')
        if len(self.traj_rir):
            if not MIN_TRAJ_STEP <= self.traj_step <= MAX_TRAJ_STEP:
                raise ValueError('traj_step must lie in %d .. %d samples' % (MIN_TRAJ_STEP, MAX_TRAJ_STEP))
            if np.any((nodes != 0) & (nodes != traj_nodes(self.length, self.traj_step))):
                raise ValueError('a moving item has exactly ceil((length - 1) / traj_step) + 1 trajectory nodes, a static one none')

    n_clips = property(lambda self: len(self.clip_start) - 1)
    n_items = property(lambda self: len(self.event))
    has_trajectories = property(lambda self: len(self.traj_rir) > 0)

    def nodes(self, i):
        """trajectory nodes of item i as a slice of the traj_* arrays (empty for a static item)"""
        return slice(int(self.traj_start[i]), int(self.traj_start[i + 1]))

    def __len__(self):
        return self.n_clips

    def clips(self, lo, hi):
        """clips lo .. hi - 1 as Scenes of their own"""
        if not 0 <= lo <= hi <= self.n_clips:
            raise IndexError((lo, hi))
        sl = slice(self.clip_start[lo], self.clip_start[hi])
        t_lo, t_hi = (int(self.traj_start[self.clip_start[k]]) for k in (lo, hi))
        return Scenes(self.n_samples, self.clip_start[lo:hi + 1] - self.clip_start[lo],
                      traj_start=self.traj_start[sl.start:sl.stop + 1] - t_lo, traj_step=self.traj_step,
                      **{f: getattr(self, f)[t_lo:t_hi] for f in self.TRAJ_FIELDS}, **{f: getattr(self, f)[sl] for f in self.FIELDS})

    def __getitem__(self, b):
        if not 0 <= b < self.n_clips:
            raise IndexError(b)
        return self.clips(b, b + 1)

    @classmethod
    def from_items(cls, n_samples, clips, pool, bank, traj_step=2400):
        """clips: per clip a list of (event, rir, onset, gain, track) -- class, length and direction come from the pool and the bank.
        `rir` is one response index, or for a moving item the list of its K trajectory nodes' indices."""
        rows = [it for clip in clips for it in clip]
        ev = np.array([r[0] for r in rows], np.int64)
        trajs = [np.asarray(r[1], np.int64).reshape(-1) if np.ndim(r[1]) else np.zeros(0, np.int64) for r in rows]
        if any(np.ndim(r[1]) and not len(t) for r, t in zip(rows, trajs)):
            raise ValueError('a trajectory holds at least one node')
        rir = np.array([t[0] if len(t) else r[1] for r, t in zip(rows, trajs)], np.int64)
        flat = np.concatenate(trajs) if trajs else np.zeros(0, np.int64)
        return cls(n_samples, np.concatenate(([0], np.cumsum([len(c) for c in clips]))), event=ev, rir=rir,
                   onset=[r[2] for r in rows], gain=[r[3] for r in rows], cls=pool.classes[ev] if len(ev) else [],
                   track=[r[4] for r in rows], length=pool.lengths[ev] if len(ev) else [],
                   azimuth=bank.azimuth[rir] if len(ev) else [], elevation=bank.elevation[rir] if len(ev) else [],
                   traj_start=np.concatenate(([0], np.cumsum([len(t) for t in trajs]))), traj_rir=flat,
                   traj_azimuth=bank.azimuth[flat], traj_elevation=bank.elevation[flat], traj_step=traj_step)


def traj_nodes(length, step):
    """K = ceil((length - 1) / step) + 1: trajectory nodes of a moving event of `length` samples (a one-sample event has one)"""
    return -(-(np.asarray(length, np.int64) - 1) // int(step)) + 1


def draw_scenes(n_clips, pool, bank, n_samples, seed, max_polyphony=2, allow_same_class=False, gain_db=(-12.0, 0.0),
                gap_s=(0.5, 4.0), fs=FS, label_rate=10, moving=0.0, speed_deg_s=(10.0, 40.0), traj_step=2400):
    """Seeded scenes: clip b draws from numpy's Generator default_rng([seed, b]).  Every track (0 .. max_polyphony - 1) is a sequence of
    events that never share a label frame, so at most max_polyphony items are active in any label frame; unless allow_same_class, an
    event whose class is active on another track in one of its label frames is drawn again (20 tries, then the place stays empty).
    Events start at a uniform gap (gap_s seconds) after the frame in which the previous one of the track ended and must fit the clip
    dry; gains are uniform in dB.
    moving: the probability that an item moves, in azimuth at its drawn response's elevation, at a speed of uniform magnitude in
    speed_deg_s (degrees per second) and either sign; node k of its trajectory is bank.nearest of the ideal point azimuth + speed k
    traj_step / fs.  With moving = 0.0 not one more random number is drawn, so every field is what it was without the keyword."""
    hop = fs // label_rate
    clips = []
    for b in range(n_clips):
        rng = np.random.default_rng([seed, b])
        items, busy = [], []                                                   # busy: (first frame, last frame, class) of every item so far
        for track in range(max_polyphony):
            cursor = int(rng.uniform(0.0, gap_s[1]) * fs)
            while True:
                placed = None
                for _ in range(20):
                    e = int(rng.integers(len(pool)))
                    ln = int(pool.lengths[e])
                    if cursor + ln > n_samples:
                        continue
                    f0, f1, k = cursor // hop, (cursor + ln - 1) // hop, int(pool.classes[e])
                    if allow_same_class or not any(c == k and f0 <= b1 and b0 <= f1 for b0, b1, c in busy):
                        placed = (e, f0, f1, k, ln)
                        break
                if placed is None:
                    if cursor + int(pool.lengths.min()) > n_samples:
                        break
                    cursor += hop
                    continue
                e, f0, f1, k, ln = placed
                g = 10.0 ** (rng.uniform(gain_db[0], gain_db[1]) / 20.0)
                r = int(rng.integers(bank.n_rirs))
                if moving > 0.0 and rng.random() < moving:
                    speed = rng.uniform(speed_deg_s[0], speed_deg_s[1]) * (1.0 if rng.random() < 0.5 else -1.0)
                    az = bank.azimuth[r] + speed * np.arange(int(traj_nodes(ln, traj_step))) * traj_step / fs
                    r = list(bank.nearest((az + 180.0) % 360.0 - 180.0, np.full(len(az), float(bank.elevation[r]))))
                items.append((e, r, cursor, g, track))
                busy.append((f0, f1, k))
                cursor = (f1 + 1) * hop + int(rng.uniform(gap_s[0], gap_s[1]) * fs)
                if cursor >= n_samples:
                    break
        items.sort(key=lambda it: (it[2], it[4]))
        clips.append(items)
    return Scenes.from_items(n_samples, clips, pool, bank, traj_step=traj_step)


def scene_rows(scene, label_rate=10, fs=FS):
    """The DCASE metadata rows (frame, class, track, azimuth, elevation) of ONE clip, int64 (n_rows, 5), sorted by frame then item.
    A moving item's row carries the direction of the trajectory node nearest the frame's centre."""
    if scene.n_clips != 1:
        raise ValueError('scene_rows takes one clip: scenes[b]')
    hop = fs // label_rate
    rows = []
    for i in range(scene.n_items):
        o, end = int(scene.onset[i]), min(int(scene.onset[i] + scene.length[i]), scene.n_samples)
        nodes, S = scene.nodes(i), scene.traj_step
        K = nodes.stop - nodes.start
        for f in range(o // hop, (end - 1) // hop + 1):
            az, el = int(scene.azimuth[i]), int(scene.elevation[i])
            if K:                                                              # the node nearest the frame's centre, a tie to the later one
                k = nodes.start + min(max((2 * (hop * f + hop // 2 - o) + S) // (2 * S), 0), K - 1)
                az, el = int(scene.traj_azimuth[k]), int(scene.traj_elevation[k])
            rows.append((f, int(scene.cls[i]), int(scene.track[i]), az, el, i))
    rows.sort(key=lambda r: (r[0], r[5]))
    return np.array([r[:5] for r in rows], np.int64).reshape(-1, 5)


def scene_labels(scene, n_frames, n_classes, label_format='classwise', label_rate=10, fs=FS):
    """Training targets of one clip over n_frames LABEL frames (rows at or past n_frames are dropped): what load_classwise_gt /
    load_trackwise_gt read from a CSV of scene_rows, by those very readers on the rows' text, hence bit for bit.  -> (sed, doa):
    classwise (n_frames, n_classes) and (n_frames, 3 n_classes); trackwise three slots per class."""
    from .dataset import LABEL_FORMATS, load_classwise_gt, load_trackwise_gt
    if label_format not in LABEL_FORMATS:
        raise ValueError('invalid label_format %r' % (label_format,))
    rows = scene_rows(scene, label_rate, fs)
    rows = rows[rows[:, 0] < n_frames]
    width = n_classes * (3 if label_format == 'trackwise' else 1)
    if not len(rows):
        return np.zeros((n_frames, width), np.float32), np.zeros((n_frames, 3 * width), np.float32)
    text = io.StringIO(''.join('%d,%d,%d,%d,%d\n' % tuple(r) for r in rows))
    if label_format == 'trackwise':
        return load_trackwise_gt(text, n_frames, n_classes, 1)[:2]
    return load_classwise_gt(text, n_frames, n_classes, 1)


def _tables(scenes, pool, bank):
    if scenes.n_items and (scenes.event.min() < 0 or scenes.event.max() >= len(pool)):
        raise ValueError('an item names no event of the pool')
    items = np.ascontiguousarray(np.stack([pool.offset[scenes.event], scenes.onset, pool.lengths[scenes.event], scenes.rir]), np.int64) \
        if scenes.n_items else np.zeros((4, 0), np.int64)
    return np.ascontiguousarray(scenes.clip_start, np.int32), items, np.ascontiguousarray(scenes.gain, np.float32)


def segment_tables(scenes, pool, bank, n_samples=None):
    """The tables salsa_scene_render_moving takes (include/salsa_hip.h).  Node k of a moving item becomes the segment of its dry samples
    ((k - 1) S, (k + 1) S) with the ramp centre k S and step S; a static item is one segment of step 0; a segment that would start at
    or past n_samples is left out.  -> (clip_start int32 (B + 1) over segments, segments int64 (6, n): source offset, onset, length,
    rir, centre from the segment's start, step; gains float32 (n); block_table int32 (B, M, 2): the first and one-past-last segment
    that reaches output block m; the longest segment)."""
    n_samples = scenes.n_samples if n_samples is None else int(n_samples)
    if scenes.n_items and (scenes.event.min() < 0 or scenes.event.max() >= len(pool)):
        raise ValueError('an item names no event of the pool')
    S = scenes.traj_step
    K = np.diff(scenes.traj_start)                                             # nodes per item, 0 for a static one
    per_item = np.maximum(K, 1)
    item = np.repeat(np.arange(scenes.n_items), per_item)                      # the item of every segment, then its node
    k = np.arange(len(item)) - np.repeat(np.cumsum(per_item) - per_item, per_item)
    moves = K[item] > 0
    ln = pool.lengths[scenes.event[item]] if len(item) else np.zeros(0, np.int64)
    a = np.where(moves, np.maximum(0, (k - 1) * S + 1), 0)
    end = np.where(moves, np.minimum(ln, (k + 1) * S), ln)
    rir = np.where(moves, scenes.traj_rir[np.where(moves, scenes.traj_start[item] + k, 0)], scenes.rir[item]) \
        if scenes.has_trajectories else scenes.rir[item]
    segs = np.stack([pool.offset[scenes.event[item]] + a, scenes.onset[item] + a, end - a, rir, np.where(moves, k * S - a, 0),
                     np.where(moves, S, 0)]).astype(np.int64) if len(item) else np.zeros((6, 0), np.int64)
    keep = segs[1] < n_samples
    segs, gains = np.ascontiguousarray(segs[:, keep]), np.ascontiguousarray(scenes.gain[item][keep], np.float32)
    first_of_item = np.concatenate(([0], np.cumsum(np.bincount(item[keep], minlength=scenes.n_items))))
    clip_start = np.ascontiguousarray(first_of_item[scenes.clip_start], np.int32)
    B, M, P, n = scenes.n_clips, -(-n_samples // PART), -(-bank.length // PART), segs.shape[1]
    first = np.repeat(clip_start[:-1].astype(np.int64), M)                     # an empty range at the clip's first segment
    last = first.copy()
    if n:
        clip_of = np.repeat(np.arange(B), np.diff(clip_start))
        m_lo = segs[1] // PART
        m_hi = np.minimum(np.minimum((segs[1] + segs[2] - 1) // PART + 1, M - 1) + P - 1, M - 1)
        # Segment s reaches blocks m_lo[s] .. m_hi[s].  Every segment reaching block m lies in [min {s: m_hi[s] >= m}, 1 + max {s: m_lo[s]
        # <= m}): two running extrema per clip instead of one entry per (segment, block); with onsets in ascending order the range is
        # tight but for segments nested inside a longer one's reach, which the kernel skips.
        s = np.arange(n)
        lo, hi = np.full((B, M), n, np.int64), np.zeros((B, M), np.int64)
        np.minimum.at(lo, (clip_of, m_hi), s)
        np.maximum.at(hi, (clip_of, m_lo), s + 1)
        lo = np.minimum.accumulate(lo[:, ::-1], axis=1)[:, ::-1].reshape(-1)
        hi = np.maximum.accumulate(hi, axis=1).reshape(-1)
        first, last = np.where(lo < hi, lo, first), np.where(lo < hi, hi, last)
    block_table = np.ascontiguousarray(np.stack([first, last], axis=-1).reshape(B, M, 2), np.int32)
    return clip_start, segs, gains, block_table, int(segs[2].max()) if n else 1


def _render_torch_fft_segments(tables, pool, bank, n_samples, ambient, out):
    """the definition composed from torch.fft calls, one per segment, each on its windowed samples (SALSA_HIP_SCENE=0); a static item is
    a segment of step 0, taken as it is"""
    import torch
    clip_start, segs, gains = tables[:3]
    dev = out.device
    ev, h = pool.on(dev), bank.rirs_on(dev)
    L = bank.length
    wet = torch.zeros_like(out)
    inside = torch.zeros((len(clip_start) - 1, 1, n_samples), dtype=torch.bool, device=dev)
    for b in range(len(clip_start) - 1):
        for i in range(clip_start[b], clip_start[b + 1]):
            src, o, ln, r, centre, step = (int(v) for v in segs[:, i])
            s = ev[src:src + ln]
            if step:                                                           # (float)(S - |q - centre|) / (float)S, one rounding of the product
                q = torch.arange(ln, device=dev)
                s = s * ((step - (q - centre).abs()).to(torch.float32) / float(step))
            full = ln + L - 1
            n_fft = 1 << (full - 1).bit_length()
            y = torch.fft.irfft(torch.fft.rfft(s, n_fft)[None] * torch.fft.rfft(h[r], n_fft), n_fft)[:, :full]
            keep = min(full, n_samples - o)
            wet[b, :, o:o + keep] += float(gains[i]) * y[:, :keep]
            inside[b, :, o:o + keep] = True
    base = ambient if ambient is not None else torch.zeros_like(out)
    out.copy_(torch.where(inside, base + wet, base))
    return out


def _launch(entry, query, host, dev, n, max_len, pool, bank, n_samples, ambient, out, device):
    """One call of the render entry point `entry`, its workspace sized by `query` for n rows of at most max_len samples.  host: the
    entry's host tables in the order of its arguments (clip_start first), dev: those of them it takes again on the device, in order."""
    import torch
    L = _lib.load()
    ws_bytes = getattr(L, query)(n_samples, max_len, n)
    ws = torch.empty(max(1, ws_bytes // 4), dtype=torch.float32, device=device)
    d_tables = [torch.from_numpy(a).to(device) for a in dev]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    hp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    with torch.cuda.device(device):
        rc = getattr(L, entry)(ptr(pool.on(device)), len(pool.flat), ptr(bank.spectra(device)), bank.n_rirs, bank.n_channels, bank.length,
                               *[hp(a) for a in host], *[ptr(t) for t in d_tables], len(host[0]) - 1, n, max_len, ptr(ambient), ptr(out),
                               n_samples, ptr(ws) if n else None, ws_bytes, C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc:
        raise RuntimeError('%s failed (%d): %s' % (entry, rc, _lib.last_error()))
    return out


def render_scenes(scenes, pool, bank, n_samples=None, ambient=None, out=None, device=None, segments=None):
    """-> CUDA float32 (B, C, n_samples).  ambient: CUDA (B, C, n_samples) or None; out may be given (and may be the ambient).
    Scenes without any trajectory go through salsa_scene_render, others through salsa_scene_render_moving; segments=True sends
    static scenes through the latter too (same bits: tests and tools/bench_scenes_moving.py compare the two)."""
    import torch
    n_samples = scenes.n_samples if n_samples is None else int(n_samples)
    B, Cn = scenes.n_clips, bank.n_channels
    if ambient is not None:
        device = ambient.device
    elif out is not None:
        device = out.device
    device = torch.device('cuda' if device is None else device)
    if out is None:
        out = torch.empty((B, Cn, n_samples), dtype=torch.float32, device=device)
    for t in (out, ambient):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (B, Cn, n_samples) and t.is_contiguous()):
            raise ValueError('render_scenes: contiguous float32 CUDA (%d, %d, %d) expected' % (B, Cn, n_samples))
    if scenes.n_items and scenes.onset.max() >= n_samples:
        raise ValueError('an onset lies outside the clip')
    as_segments = scenes.has_trajectories or bool(segments)
    if not as_segments and np.diff(scenes.clip_start).max() > MAX_ITEMS_PER_CLIP:
        raise ValueError('a clip holds at most %d items' % MAX_ITEMS_PER_CLIP)
    if as_segments or not HIP_SCENE:                                           # the torch.fft leg takes static items as segments of step 0
        tables = segment_tables(scenes, pool, bank, n_samples)
        clip_start, segs, gains, block_table, max_seg = tables
        if as_segments and np.diff(clip_start).max() > MAX_SEGMENTS_PER_CLIP:
            raise ValueError('a clip holds at most %d segments' % MAX_SEGMENTS_PER_CLIP)
        if not HIP_SCENE:
            return _render_torch_fft_segments(tables, pool, bank, n_samples, ambient, out)
        return _launch('salsa_scene_render_moving', 'salsa_scene_moving_workspace_bytes', (clip_start, segs, gains, block_table),
                       (segs, gains, block_table), segs.shape[1], max_seg, pool, bank, n_samples, ambient, out, device)
    tables = _tables(scenes, pool, bank)
    return _launch('salsa_scene_render', 'salsa_scene_workspace_bytes', tables, tables, scenes.n_items, pool.max_len, pool, bank,
                   n_samples, ambient, out, device)


def add_scenes(feature_bank, scenes, pool, bank, names=None, ambient=None, n_classes=None, label_rate=10, fs=FS, diffuse=None):
    """Render, then feature_bank.add_clips(audio, names, sed=, doa=) with the scenes' labels in the bank's label format.  -> the audio.
    diffuse: (DiffuseField, dict(snr_db= or level_db=, seed=)) adds spatially diffuse noise to the render (ambient.add_diffuse, DESIGN.md
    section 9q; clip b gets the seed `seed` + b); None leaves the render as it is."""
    audio = render_scenes(scenes, pool, bank, ambient=ambient, device=feature_bank.device)
    if diffuse is not None:
        from . import ambient as _ambient
        field, how = diffuse
        if field.audio_format != bank.audio_format:
            raise ValueError('a %s field on a %s bank' % (field.audio_format, bank.audio_format))
        how = dict(how)
        _ambient.add_diffuse(audio, field, seeds=how.pop('seed', None), out=audio, **how)
    fmt = feature_bank.label_format
    n_classes = (feature_bank.n_classes // 3 if fmt == 'trackwise' else feature_bank.n_classes) if n_classes is None else n_classes
    n_lab = -(-scenes.n_samples // (fs // label_rate))
    labels = [scene_labels(scenes[b], n_lab, n_classes, fmt, label_rate, fs) for b in range(scenes.n_clips)]
    names = ['scene_%04d' % b for b in range(scenes.n_clips)] if names is None else list(names)
    feature_bank.add_clips(audio, names, sed=[lab[0] for lab in labels], doa=[lab[1] for lab in labels])
    return audio


_ROOMS = ('ShoeboxRoom', 'RoomImages', 'room_images', 'room_rirs', 'room_rir_bank', 'eyring_beta', 'RirAcoustics', 'rir_acoustics',
          'calibrate_room', 'sphere_response', 'sphere_filter', 'SphereTable', 'sphere_table', 'OCTAVE_BANDS', 'octave_filters')
_AMBIENT = ('DiffuseField', 'diffuse_noise', 'add_diffuse', 'colour_filter', 'fibonacci_sphere')


def __getattr__(name):
    """rooms.py (DESIGN.md sections 9m - 9p: image-source responses of a shoebox room as a RirBank, their decay, the rigid sphere, octave-band walls) builds on this module, so its public names
    are re-exported on first use, not at import"""
    if name in _ROOMS:
        from . import rooms
        return getattr(rooms, name)
    if name in _AMBIENT:                                                       # ambient.py (diffuse noise) likewise
        from . import ambient
        return getattr(ambient, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
