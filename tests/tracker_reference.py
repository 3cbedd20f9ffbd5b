"""The noise-floor tracker (K2, tracker_kernel) restated in plain numpy float64, and the seeded spectrogram blocks that
tests/test_tracker_cpu.py and tests/test_tracker_gpu.py hold it to.

tracker_mask() follows the tracker of the reference's extract_normalized_eigenvector (salsa_feature_extraction.py:28-87):
power of channel 0, the 3-frame sum over the wrapped time axis in the order ((0 + p[t]) + p[t-1]) + p[t-2], / 3, square
root; initial floor 0.5 * mean(mag[:, 0:5]); per frame the strict `mag > floor`, the countdown from 3, x 1.02 / x 1.002 /
x 0.98, the 1e-6 clamp and the strict `mag > ratio * floor`.  Vectorised over every leading axis (clips, bins), looping
over frames.

CASES is the table both test files run.  Columns: name, family, clips, bins, frames, seed, and the deliberate changes of
the restatement (MUTANTS) that this case's mask must expose.  Every clip of a batch is its own track (seed, clip index).
The union of the shapes holds the frame counts {1..6, 63..65, 127..129, 191..193, 4801} and the bin counts
{1, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 191, 200}; batches are 1, 3, 4 and 32."""
import functools

import numpy as np

TR_CH = 64          # frames per chunk of tracker_kernel
TR_BINS = 32        # bins per workgroup / mask word

# one deliberate change each; tracker_mask(mutate=...) must then differ from the plain restatement on a committed case
MUTANTS = ('ge', 'countdown_le0', 'clamp_first', 'nowrap', 'floor32')


def tracker_mask(X, power='hypot', ratio=1.5, raw=False, trace=False, mutate=None):
    """X complex (..., n_bins, n_frames, n_ch) -> bool indicator_sig (..., n_bins, n_frames) [, trace dict].

    power: 'hypot' |X0|^2 as np.abs(X0) ** 2 (the reference, the C oracle); 'sumsq' re * re + im * im (the kernel).
    raw: track |X0| itself with a clamped initial floor (the contrib tracker; nothing asserts on it yet).
    trace: also return per-frame float64 / int / bool arrays: mag, floor_before, floor, countdown, above, slow, clamped
           (slow: the x 1.002 step was taken; clamped: the product fell below 1e-6 and the clamp acted)."""
    assert mutate is None or mutate in MUTANTS
    x0 = np.asarray(X)[..., 0]
    lead, T = x0.shape[:-1], x0.shape[-1]
    x0 = x0.reshape(-1, T).astype(np.complex128)
    if power == 'hypot':
        p = np.abs(x0) ** 2
    else:
        assert power == 'sumsq'
        p = x0.real * x0.real + x0.imag * x0.imag
    if raw:
        mag = np.sqrt(p)
    else:
        acc = np.zeros_like(p)
        for k in range(3):
            idx = np.arange(T) - k
            pk = p[:, idx % T]
            if mutate == 'nowrap':
                pk = np.where(idx[None, :] < 0, 0.0, pk)
            acc = acc + pk
        mag = np.sqrt(acc / 3)
    n0 = min(5, T)
    acc0 = np.zeros(mag.shape[0])
    for t in range(n0):
        acc0 = acc0 + mag[:, t]
    floor = 0.5 * (acc0 / n0)
    if raw:
        floor = np.maximum(floor, 1e-6)
    countdown = np.full(mag.shape[0], 3, dtype=np.int64)
    up, up_slow, down = 1 + 0.02, 1 + 0.1 * 0.02, 1 - 0.02
    mask = np.zeros(mag.shape, dtype=bool)
    tr = None
    if trace:
        tr = dict(mag=mag, floor_before=np.zeros_like(mag), floor=np.zeros_like(mag),
                  countdown=np.zeros(mag.shape, np.int64), above=np.zeros(mag.shape, bool),
                  slow=np.zeros(mag.shape, bool), clamped=np.zeros(mag.shape, bool))
    for t in range(T):
        m = mag[:, t]
        above = m >= floor if mutate == 'ge' else m > floor
        countdown = np.where(above, countdown - 1, 3)
        slow = above & (countdown <= 0 if mutate == 'countdown_le0' else countdown < 0)
        factor = np.where(above, np.where(slow, up_slow, up), down)
        if trace:
            tr['floor_before'][:, t] = floor
        if mutate == 'clamp_first':
            prod = factor * np.maximum(floor, 1e-6)
            clamped = np.zeros_like(above)
            floor = prod
        else:
            prod = factor * floor
            clamped = prod < 1e-6
            floor = np.where(clamped, 1e-6, prod)
        if mutate == 'floor32':
            floor = floor.astype(np.float32).astype(np.float64)
        mask[:, t] = m >= ratio * floor if mutate == 'ge' else m > ratio * floor
        if trace:
            tr['floor'][:, t] = floor
            tr['countdown'][:, t] = countdown
            tr['above'][:, t] = above
            tr['slow'][:, t] = slow
            tr['clamped'][:, t] = clamped
    mask = mask.reshape(lead + (T,))
    if trace:
        return mask, {k: v.reshape(lead + (T,)) for k, v in tr.items()}
    return mask


# ------------------------------------------------------------------------------------------------------ track builders
def _block(x0, rng):
    """channel 0 (n_bins, n_frames) real or complex -> complex64 (n_bins, n_frames, 4); channels 1-3 only feed the solver"""
    nb, T = x0.shape
    X = np.empty((nb, T, 4), np.complex64)
    X[..., 0] = x0
    o = rng.standard_normal((nb, T, 3, 2), dtype=np.float32)
    X[..., 1:] = 0.1 * (o[..., 0] + 1j * o[..., 1])
    return X


def _levels(rng, nb, T, decades=(-7.5, -1.5)):
    """per-bin level spread over six decades times a loud / quiet gain that switches frame-wise"""
    level = 10.0 ** rng.uniform(decades[0], decades[1], (nb, 1))
    state = np.cumsum(rng.random((nb, T)) < 0.08, axis=1) % 2 == 0
    return level * np.where(state, 1.0, 0.03)


def build_random(seed, nb, T):
    rng = np.random.default_rng([seed, 1])
    g = rng.standard_normal((nb, T, 2), dtype=np.float32)
    return _block(_levels(rng, nb, T) * (g[..., 0] + 1j * g[..., 1]), rng), {}


def build_realonly(seed, nb, T):
    rng = np.random.default_rng([seed, 2])
    return _block(_levels(rng, nb, T) * rng.standard_normal((nb, T), dtype=np.float32), rng), {}


def build_silent(seed, nb, T):
    rng = np.random.default_rng([seed, 3])
    return _block(np.zeros((nb, T)), rng), {}


def _near(v):
    v = np.float32(v)
    return [float(np.nextafter(v, np.float32(0))), float(v), float(np.nextafter(v, np.float32(1)))]


# at, just above and just below the clamp, 1.5 x the clamp and 4e-6 (the dormant TR_CHUNK_CLAMP_SKIP test); 2.27e-6 after a
# 0.99e-6 plateau gives a 3-frame RMS of 1.54e-6, between 1.5 x 1.02e-6 and 1.5 x 1.02^2 e-6
CLAMP_MENU = ([0.0, 0.98e-6, 0.99e-6, 1.01e-6, 1.49e-6, 1.51e-6, 1.54e-6, 2.27e-6, 3.9e-6, 4.1e-6, 1e-5, 1e-3, 1.0]
              + _near(1e-6) + _near(1.5e-6) + _near(4e-6))


DECAY_BOUNDARY = 11 * TR_CH     # a floor of about 0.4 needs 640 steps of x 0.98 to reach 1e-6: the first boundary it can be aimed at


def _first_clamp(n, amp, T=DECAY_BOUNDARY + 96):
    """frame on which the clamp first acts for a row that is amp on frames [0, n) and silent after (its last two frames included)"""
    row = np.zeros(T, np.float32)
    row[:n] = amp
    return int(np.argmax(_row_eval(row)[1]['clamped'][0]))


@functools.lru_cache(maxsize=None)
def _burst_for_first_clamp(frame):
    """(n, amp): the first clamped frame moves by one or two per loud frame, so a second level fills the gaps"""
    for n in range(40, 70):
        for amp in (1.0, 0.99, 0.97, 0.95):
            if _first_clamp(n, amp) == frame:
                return n, amp
    raise AssertionError('no burst puts the first clamped frame on %d' % frame)


def build_clamp(seed, nb, T):
    """Real channel 0.  Every bin but bin 0 is silent for its first five frames and its last two, so its floor starts at exactly 0.
    bin 0: silent; in a long clip 1.0 up to frame 2000 and silent after, so its floor decays from about 1 onto the clamp (0.98^680)
    long before the last full chunk hands over to the ragged tail.  bin 1: silent up to frame 130 (the clamp acts on 63, 64, 127, 128), then
    the menu.  bin 2: plateaus of 0.99e-6 with 2.27e-6 blips.  bins 3, 4 of a long clip: loud for just so many frames from frame 0 that
    the decaying floor FIRST meets the clamp on frame 703 / 704, the last frame of a full chunk / the first of the next.  The rest: silences and short plateaus drawn from CLAMP_MENU."""
    rng = np.random.default_rng([seed, 4])
    a = np.zeros((nb, T))
    long_clip = T >= 4000 and nb > 4
    first_clamp = [(3, DECAY_BOUNDARY - 1), (4, DECAY_BOUNDARY)] if long_clip else []
    for b in range(nb):
        if b == 0:
            if T >= 4000:
                a[0, :2000] = 1.0
            continue
        if long_clip and b in (3, 4):
            n, amp = _burst_for_first_clamp(first_clamp[b - 3][1])
            a[b, :n] = amp
            continue
        t = 130 if b == 1 else int(rng.integers(5, 70))
        while t < T - 2:
            if b == 2:
                n, v = int(rng.integers(4, 9)), 0.99e-6
                a[b, t:t + n] = v
                if t + n < T - 2:
                    a[b, t + n] = 2.27e-6
                t += n + 1
                continue
            if rng.random() < 0.25:
                n, v = int(rng.integers(3, 40)), 0.0
            else:
                n, v = int(rng.integers(1, 12)), CLAMP_MENU[int(rng.integers(len(CLAMP_MENU)))]
            a[b, t:t + n] = v
            t += n
        a[b, T - 2:] = 0.0
    sign = np.where(rng.random((nb, T)) < 0.5, -1.0, 1.0)
    last_full = TR_CH * (T // TR_CH) - 1
    info = dict(clamp_frames=[(1, t) for t in (63, 64, 127, 128) if t < min(T, 130)]
                + ([(0, last_full), (0, last_full + 1)] if T >= 4000 and T % TR_CH else []), first_clamp=first_clamp)
    return _block((a * sign).astype(np.float32), rng), info


def build_slowrise(seed, nb, T):
    """Real channel 0 at a quiet level q with, before every chunk boundary 64 j, four silent frames (mag = 0 on the last: not
    `above`) and a burst of 1.0 from frame s = 64 j - k, k = bin % 4 + 1: `above` from s on, first x 1.002 step on s + 3 =
    64 j - 1, 64 j, 64 j + 1, 64 j + 2.  Bins with (bin // 4) % 3 == 1 / 2 instead start the burst at 64 j - 8 and go silent for the
    three frames ending at d = 64 j - 1 / 64 j: mag = 0 on d alone, a one-frame dip that resets the countdown; first slow step d + 4."""
    rng = np.random.default_rng([seed, 5])
    a = np.zeros((nb, T))
    slow, dips = [], []
    for b in range(nb):
        q = 1e-3 * (1 + b % 5)
        a[b] = q
        k, variant = b % 4 + 1, (b // 4) % 3
        for j in range(1, (T - 24) // TR_CH + 1):
            if variant == 0:
                s = TR_CH * j - k
                a[b, s - 4:s], a[b, s:s + 14], a[b, s + 14:s + 18] = 0.0, 1.0, 0.0
                slow.append((b, s, s + 3))
            else:
                s, d = TR_CH * j - 8, TR_CH * j - 1 + (variant - 1)
                a[b, s - 4:s], a[b, s:s + 22], a[b, s + 22:s + 26] = 0.0, 1.0, 0.0
                a[b, d - 2:d + 1] = 0.0
                dips.append((b, d))
                slow.append((b, d + 1, d + 4))
    sign = np.where(rng.random((nb, T)) < 0.5, -1.0, 1.0)
    return _block((a * sign).astype(np.float32), rng), dict(slow=slow, dips=dips)


def build_wrap(seed, nb, T):
    """Real channel 0 at moderate levels; the last two frames are 300 x louder (odd bins) or 300 x quieter (even bins) than the
    rest, so frames 0 and 1 and the initial floor are decided by the wrapped frames."""
    rng = np.random.default_rng([seed, 6])
    a = 10.0 ** rng.uniform(-3, -1, (nb, 1)) * (0.3 + rng.random((nb, T))) * np.where(rng.random((nb, T)) < 0.5, -1.0, 1.0)
    a[:, max(T - 2, 0):] *= np.where(np.arange(nb) % 2 == 1, 300.0, 1 / 300.0)[:, None]
    return _block(a.astype(np.float32), rng), {}


def _row_eval(row, mutate=None):
    X = np.zeros((1, row.size, 4), np.complex64)
    X[0, :, 0] = row
    return tracker_mask(X, trace=True, mutate=mutate)


def _f32_step(v, n):
    return (np.float32(v).view(np.int32) + np.int32(n)).view(np.float32)


# The exact tie is the only input in the table that tells `>` from `>=` (MUTANTS 'ge'): one-ulp neighbours pass either way and so
# does 0 > 0, whose countdown is reset on the next silent frame.  test_tracker_cpu.py asserts mag == floor from the trace.
def _solve_tie(F):
    """float32 (a, b, c) with sqrt((((0 + a a) + b b) + c c) / 3) == F in float64, a >> b >> c; None if the search fails"""
    s0 = 3.0 * F * F
    for ds in (0, 1, -1, 2, -2, 3, -3):
        s = s0
        for _ in range(abs(ds)):
            s = np.nextafter(s, np.inf if ds > 0 else 0.0)
        if np.sqrt(np.float64(s) / 3) != F:
            continue
        a = np.float32(np.sqrt(s))
        while float(a) ** 2 > s:
            a = np.nextafter(a, np.float32(0))
        r1 = s - float(a) ** 2
        b0 = np.float32(np.sqrt(r1))
        while float(b0) ** 2 > r1:
            b0 = np.nextafter(b0, np.float32(0))
        for j in range(256):
            b = _f32_step(b0, -j)
            r2 = r1 - float(b) ** 2
            c0 = np.float32(np.sqrt(r2))
            for c in (c0, np.nextafter(c0, np.float32(0)), np.nextafter(c0, np.float32(np.inf))):
                if ((0.0 + float(a) ** 2) + float(b) ** 2) + float(c) ** 2 == s:
                    return a, b, c
    return None


KNIFE_T = 196      # three full chunks and a ragged tail of four frames
KNIFE_TARGETS = (('floor', 20), ('floor', 64), ('floor', 65), ('floor', 128), ('floor', 192),
                 ('sig', 21), ('sig', 66), ('sig', 129), ('sig', 195), ('tie', 30), ('tie', 70))


def _knife_rows(kind, t0, rng):
    """-> rows (1 or 2, KNIFE_T) float32 for one target, or None where this draw does not give the property (the caller redraws)"""
    T = KNIFE_T
    row = (1e-2 * (0.5 + rng.random(T)) * np.where(rng.random(T) < 0.5, -1.0, 1.0)).astype(np.float32)
    if kind == 'tie':
        row[t0 - 1], row[t0 - 2] = row[t0] * 2.0 ** -12, row[t0] * 2.0 ** -24
        F = _row_eval(row)[1]['floor_before'][0, t0]
        sol = _solve_tie(F)
        if sol is None:
            return None
        row[t0], row[t0 - 1], row[t0 - 2] = sol
        _, tr = _row_eval(row)
        if tr['mag'][0, t0] != F or tr['floor_before'][0, t0] != F:
            return None
        b2 = 3 * (1.53 * F) ** 2 - float(row[t0]) ** 2 - float(row[t0 - 1]) ** 2
        row[t0 + 1] = np.sqrt(b2)
        m, m_ge = _row_eval(row)[0], _row_eval(row, 'ge')[0]
        if np.array_equal(m, m_ge) or not np.array_equal(m[0, :t0], m_ge[0, :t0]):
            return None
        return row[None]
    row[t0 - 1] *= 0.2
    row[t0 - 2] *= 0.2

    def bit(v):
        r = row.copy()
        r[t0] = v
        m, tr = _row_eval(r)
        return bool(tr['above'][0, t0] if kind == 'floor' else m[0, t0])

    lo, hi = np.float32(0).view(np.int32), np.float32(10).view(np.int32)
    if bit(np.float32(0)) or not bit(np.float32(10)):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bit(mid.view(np.float32)):
            hi = mid
        else:
            lo = mid
    pair = np.stack([row, row])
    pair[0, t0], pair[1, t0] = lo.view(np.float32), hi.view(np.float32)
    if kind == 'floor':     # the next frame's RMS between 1.5 x the two floors that the compare decides between
        F = _row_eval(pair[0])[1]['floor_before'][0, t0]
        b2 = 3 * (1.53 * F) ** 2 - float(pair[0, t0]) ** 2 - float(pair[0, t0 - 1]) ** 2
        if b2 <= 0:
            return None
        pair[:, t0 + 1] = np.sqrt(b2)
    (m0, tr0), (m1, tr1) = _row_eval(pair[0]), _row_eval(pair[1])
    diff = np.flatnonzero(m0[0] != m1[0])
    if kind == 'sig' and diff.tolist() != [t0]:
        return None
    if kind == 'floor' and (tr0['above'][0, t0] or not tr1['above'][0, t0] or diff.size == 0 or diff[0] < t0
                            or not np.array_equal(tr0['above'][0, :t0], tr1['above'][0, :t0])):
        return None
    return pair


def build_knife(seed, nb=None, T=KNIFE_T):
    """Real channel 0.  Per target (compare, frame) two bins whose channel-0 amplitude at that frame are ADJACENT float32 values
    with different outcomes of `mag > floor` ('floor': the masks then part on the next frame) or of `mag > 1.5 floor` ('sig': that
    mask bit alone differs).  'tie': one bin whose 3-frame RMS EQUALS its floor at that frame in float64 (amplitudes solved for by
    _solve_tie), so only the strictness of the compare decides.  Targets: first chunk, on and after a boundary, the ragged tail."""
    assert T == KNIFE_T
    rng = np.random.default_rng([seed, 7])
    rows, targets = [], []
    for kind, t0 in KNIFE_TARGETS:
        for _ in range(200):
            r = _knife_rows(kind, t0, rng)
            if r is not None:
                break
        else:
            raise AssertionError('no %s knife edge found at frame %d' % (kind, t0))
        targets.append((kind, t0, tuple(range(len(rows), len(rows) + len(r)))))
        rows.extend(r)
    X = _block(np.stack(rows), rng)
    assert nb is None or nb == X.shape[0]
    return X, dict(targets=targets)


KNIFE_BINS = sum(1 if k == 'tie' else 2 for k, _ in KNIFE_TARGETS)

BUILDERS = dict(random=build_random, realonly=build_realonly, silent=build_silent, clamp=build_clamp,
                slowrise=build_slowrise, wrap=build_wrap, knife=build_knife)

# name, family, clips, bins, frames, seed, mutants this case must expose
CASES = (
    ('rand_33x1', 'random', 1, 33, 1, 11, ('nowrap',)),
    ('rand_31x2', 'random', 1, 31, 2, 12, ('nowrap',)),
    ('rand_32x3', 'random', 1, 32, 3, 13, ('nowrap',)),
    ('rand_b3_63x4', 'random', 3, 63, 4, 14, ('countdown_le0', 'nowrap')),
    ('rand_64x5', 'random', 1, 64, 5, 15, ()),
    ('rand_65x6', 'random', 1, 65, 6, 16, ()),
    ('rand_96x63', 'random', 1, 96, 63, 17, ('countdown_le0', 'clamp_first', 'nowrap')),
    ('rand_127x64', 'random', 1, 127, 64, 18, ()),
    ('rand_b3_128x65', 'random', 3, 128, 65, 19, ()),
    ('rand_129x127', 'random', 1, 129, 127, 20, ()),
    ('rand_191x128', 'random', 1, 191, 128, 21, ()),
    ('rand_200x129', 'random', 1, 200, 129, 22, ('countdown_le0',)),
    ('rand_1x191', 'random', 1, 1, 191, 23, ()),
    ('rand_33x192', 'random', 1, 33, 192, 24, ()),
    ('rand_b4_200x4801', 'random', 4, 200, 4801, 25, ()),
    ('rand_b32_200x4801', 'random', 32, 200, 4801, 26, ()),
    ('real_129x193', 'realonly', 1, 129, 193, 31, ('countdown_le0', 'clamp_first', 'nowrap')),
    ('real_b3_191x129', 'realonly', 3, 191, 129, 32, ()),
    ('silent_33x65', 'silent', 1, 33, 65, 41, ()),
    ('clamp_33x129', 'clamp', 1, 33, 129, 42, ('clamp_first',)),
    ('clamp_65x4801', 'clamp', 1, 65, 4801, 43, ('clamp_first',)),
    ('slowrise_33x193', 'slowrise', 1, 33, 193, 51, ('countdown_le0',)),
    ('knife_%dx196' % KNIFE_BINS, 'knife', 1, KNIFE_BINS, KNIFE_T, 61, ('ge', 'countdown_le0', 'floor32')),
    ('wrap_32x5', 'wrap', 1, 32, 5, 71, ('nowrap',)),
    ('wrap_b3_33x4', 'wrap', 3, 33, 4, 72, ('nowrap',)),
    ('wrap_63x6', 'wrap', 1, 63, 6, 73, ('nowrap',)),
    ('wrap_31x65', 'wrap', 1, 31, 65, 74, ('nowrap',)),
)
CASE_NAMES = tuple(c[0] for c in CASES)
ALL_SILENT = 'silent_33x65'
SOLVER_SUBSET = ('rand_b4_200x4801', 'clamp_65x4801', 'slowrise_33x193')     # also through the production solver's mask read
# small blocks (at most 70 bins x 200 frames: the reference loops in Python over every bin) whose masks fixture g27 holds as the
# reference itself computes them
GOLDEN_CASES = ('rand_33x1', 'rand_31x2', 'rand_32x3', 'rand_b3_63x4', 'rand_65x6', 'rand_33x192', 'silent_33x65', 'clamp_33x129',
                'slowrise_33x193', 'knife_%dx196' % KNIFE_BINS, 'wrap_32x5', 'wrap_b3_33x4', 'wrap_63x6', 'wrap_31x65')
FORMAT_SUBSET = ('rand_b3_128x65', 'real_129x193', 'clamp_33x129', 'knife_%dx196' % KNIFE_BINS)   # FOA and MIC see one mask


def case(name):
    return CASES[CASE_NAMES.index(name)]


def build_case(name):
    """-> X complex64 (clips, bins, frames, 4), [info dict per clip]"""
    _, family, B, nb, T, seed, _ = case(name)
    built = [BUILDERS[family](1000 * seed + clip, nb, T) for clip in range(B)]
    X = np.stack([x for x, _ in built])
    assert X.shape == (B, nb, T, 4) and X.dtype == np.complex64
    return X, [i for _, i in built]


def describe_first_difference(got, want, X):
    """text for an assertion: the first differing (clip, bin, frame), its chunk and the restatement's state there"""
    d = np.argwhere(got != want)
    if d.size == 0:
        return 'no difference'
    c, b, t = (int(v) for v in d[0])
    _, tr = tracker_mask(X[c, b:b + 1], trace=True)
    return ('%d differing bits; first at clip %d bin %d (32-bin group %d, bit %d) frame %d (chunk %d, offset %d): got %d want %d; '
            'mag %.17g floor before %.17g after %.17g countdown %d above %d'
            % (len(d), c, b, b // TR_BINS, b % TR_BINS, t, t // TR_CH, t % TR_CH, got[c, b, t], want[c, b, t],
               tr['mag'][0, t], tr['floor_before'][0, t], tr['floor'][0, t], tr['countdown'][0, t], tr['above'][0, t]))
