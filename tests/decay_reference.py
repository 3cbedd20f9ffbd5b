"""Float64 restatement of the decay measurement (include/salsa_hip.h: salsa_rir_decay) for the tests, one
response at a time, and the input families the tests measure.

    e[n] = h[n]^2 (exact in float64 for float32 h),  EDC[n] = sum_{m >= n} e[m],  E = EDC[0],  n_d = the first index of the largest |h|,
    i(x) = the first n with EDC[n] <= E 10^(x / 10), x in LEVELS_DB,
    EDT / T20 / T30 = -60 / slope of the least-squares line through (n / fs, 10 log10(EDC[n] / E)), n in [i(lo), i(hi)], centred sums,
    headroom = -(slope per tap) (L - 1 - i(hi)),  DRR and C50 from sums of e over the taps around and after n_d.

measure(h, order='fsum') is the reference: every sum is correctly rounded -- math.fsum, and for the L suffix sums of the curve exact
integer arithmetic (e 2^298 is a whole number for every float32 h), which gives what math.fsum(e[n:]) gives without L^2 work.
order='forward' and order='reverse' are the YARDSTICKS: the same definition with plain float64 additions in two different orders (the
curve as a running sum from the last tap, or in runs of 61 taps with a scan of the runs' totals; every other sum over ascending or
descending taps).  How far they land from the reference is the error any float64 evaluation may show (section 9j's convention).

margin(result): the knife-edge margin of the case, min |EDC[n] / threshold - 1| over n = i(x) and i(x) - 1 and the four levels below
0 dB (the level 0 dB is crossed at tap 0 by definition: EDC[0] = E in any arithmetic).  A case is only used when this exceeds
MIN_MARGIN = 1e-9, far above any float64 summation error (L 2^-53 = 1.8e-12 at most), so that no evaluation can find another index."""
import fractions
import functools
import math

import numpy as np

FS = 24000.0
LEVELS_DB = (0.0, -5.0, -10.0, -25.0, -35.0)
FITS = (('edt', 0, 2), ('t20', 1, 3), ('t30', 1, 4))
NAMES = ('energy', 'peak', 'edt', 't20', 't30', 'headroom_edt', 'headroom_t20', 'headroom_t30', 'drr_db', 'c50_db',
         'cross_0db', 'cross_5db', 'cross_10db', 'cross_25db', 'cross_35db')
IDX = {n: i for i, n in enumerate(NAMES)}
EXACT = ('peak', 'cross_0db', 'cross_5db', 'cross_10db', 'cross_25db', 'cross_35db')      # held bit for bit
FITTED = ('edt', 't20', 't30', 'headroom_edt', 'headroom_t20', 'headroom_t30', 'drr_db', 'c50_db')
MIN_MARGIN = 1e-9
_SHIFT = 298                                                                   # the smallest square of a float32 is 2^-298


def halfwidth(fs=FS):
    return int(math.floor(0.0025 * fs + 0.5))


def _total(values, order):
    values = [float(v) for v in values]
    if order == 'fsum':
        return math.fsum(values)
    acc = 0.0
    for v in (values if order == 'forward' else reversed(values)):
        acc += v
    return acc


def curve(e, order='fsum'):
    """EDC of the energies e (float64, >= 0)"""
    L = len(e)
    out = np.zeros(L, np.float64)
    if order == 'fsum':
        scaled = e * 2.0 ** _SHIFT
        assert np.all(np.isfinite(scaled))
        if np.all(scaled == np.floor(scaled)):                                 # squares of float32 values
            acc, one = 0, 1 << _SHIFT
            for n in range(L - 1, -1, -1):
                acc += int(scaled[n])
                out[n] = acc / one                                             # int / int: correctly rounded
        else:                                                                  # any float64 energies (the closed-form checks)
            acc = fractions.Fraction(0)
            for n in range(L - 1, -1, -1):
                acc += fractions.Fraction(float(e[n]))
                out[n] = float(acc)                                            # correctly rounded as well
    elif order == 'forward':
        out[:] = np.cumsum(e[::-1])[::-1]                                      # one running sum from the last tap
    else:
        run, off = 61, 0.0
        for lo in range(((L - 1) // run) * run, -1, -run):
            local = np.cumsum(e[lo:lo + run][::-1])[::-1]
            out[lo:lo + run] = off + local
            off = off + local[0]
    return out


def measure(h, fs=FS, direct_halfwidth=None, order='fsum'):
    """-> dict(params float64 (15) in NAMES' order, edc float64 (L), thresholds (5))"""
    h = np.asarray(h)
    assert h.ndim == 1 and len(h) >= 1
    L, nan = len(h), float('nan')
    hw = halfwidth(fs) if direct_halfwidth is None else int(direct_halfwidth)
    e = h.astype(np.float64) ** 2
    edc = curve(e, order)
    E = float(edc[0])
    p = np.full(len(NAMES), nan)
    p[IDX['energy']], p[IDX['peak']] = E, 0.0
    if not E > 0:
        p[IDX['energy']] = 0.0
        return dict(params=p, edc=edc, thresholds=[0.0] * 5)
    mag = np.abs(h)
    n_d = int(np.nonzero(mag == mag.max())[0][0])
    p[IDX['peak']] = n_d
    thresholds = [E * 10.0 ** (x / 10.0) for x in LEVELS_DB]
    cross = []
    for k, thr in enumerate(thresholds):
        at = np.nonzero(edc <= thr)[0]
        cross.append(int(at[0]) if len(at) else None)
        p[IDX['cross_0db'] + k] = nan if cross[k] is None else cross[k]
    for name, lo, hi in FITS:
        i0, i1 = cross[lo], cross[hi]
        if i1 is None or not edc[i1] > 0 or i1 - i0 + 1 < 2:
            continue
        ns = range(i0, i1 + 1)
        x = [n / fs for n in ns]
        y = [10.0 * math.log10(edc[n] / E) for n in ns]
        xbar, ybar = _total(x, order) / len(x), _total(y, order) / len(y)
        sxy = _total([(a - xbar) * (b - ybar) for a, b in zip(x, y)], order)
        sxx = _total([(a - xbar) ** 2 for a in x], order)
        slope = sxy / sxx                                                      # dB per second
        p[IDX[name]] = -60.0 / slope
        p[IDX['headroom_' + name]] = -(slope / fs) * (L - 1 - i1)
    direct = [e[n] for n in range(L) if abs(n - n_d) <= hw]
    rest = [e[n] for n in range(L) if abs(n - n_d) > hw]
    n_e = n_d + int(math.floor(0.05 * fs + 0.5))
    e_dir, e_rest = _total(direct, order), _total(rest, order)
    e_early, e_late = _total(e[:n_e], order), _total(e[n_e:], order)
    p[IDX['drr_db']] = 10.0 * math.log10(e_dir / e_rest) if e_rest > 0 else float('inf')
    p[IDX['c50_db']] = 10.0 * math.log10(e_early / e_late) if e_late > 0 else float('inf')
    return dict(params=p, edc=edc, thresholds=thresholds)


def margin(result):
    """the knife-edge margin of a measured case (1.0 for a silent response)"""
    edc, worst = result['edc'], 1.0
    if not result['params'][IDX['energy']] > 0:
        return worst
    for k in range(1, len(LEVELS_DB)):
        thr, i = result['thresholds'][k], result['params'][IDX['cross_0db'] + k]
        at = [len(edc) - 1] if np.isnan(i) else [int(i)] + ([int(i) - 1] if i >= 1 else [])
        worst = min([worst] + [abs(float(edc[n]) / thr - 1.0) for n in at])
    return worst


def measure_case(h, fs=FS, direct_halfwidth=None):
    """The reference and the two yardsticks of one response -> (reference result, Y (15): the larger distance of a yardstick from the
    reference per parameter, NaN and inf patterns asserted equal, margin).  Asserts on the reference alone; never on code under test."""
    ref = measure(h, fs, direct_halfwidth)
    yard = [measure(h, fs, direct_halfwidth, order) for order in ('forward', 'reverse')]
    m = margin(ref)
    Y = np.zeros(len(NAMES))
    if m > MIN_MARGIN:
        for y in yard:
            a, b = ref['params'], y['params']
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), 'a yardstick disagrees on validity'
            for name in EXACT:
                assert a[IDX[name]] == b[IDX[name]] or (np.isnan(a[IDX[name]]) and np.isnan(b[IDX[name]])), name
            fin = np.isfinite(a)
            Y[fin] = np.maximum(Y[fin], np.abs(a[fin] - b[fin]))
    return ref, Y, m


# ---- input families ------------------------------------------------------------------------------------------------------------------
def geometric(L, T=0.3, fs=FS, dtype=np.float32):
    """h[n] = r^n, r = 10^(-3 / (T fs)): 60 dB of decay per T seconds"""
    return (10.0 ** (-3.0 * np.arange(L, dtype=np.float64) / (T * fs))).astype(dtype)


def geometric_edc(L, T=0.3, fs=FS):
    """the closed form of geometric's curve: r^(2n) (1 - r^(2 (L - n))) / (1 - r^2)"""
    n = np.arange(L, dtype=np.float64)
    r2 = 10.0 ** (-6.0 / (T * fs))
    return r2 ** n * (1.0 - r2 ** (L - n)) / (1.0 - r2)


def two_slope(L, seed):
    rng = np.random.RandomState(seed)
    sign = np.where(rng.rand(L) < 0.5, -1.0, 1.0)
    return (sign * (0.8 * geometric(L, 0.1, dtype=np.float64) + 0.2 * geometric(L, 0.6, dtype=np.float64))).astype(np.float32)


def impulse(L, at, value=1.0):
    h = np.zeros(L, np.float32)
    h[at] = value
    return h


def decay_then_zeros(L, seed):
    """a noisy 0.3-s decay cut to exact zeros where its level is about -15 dB (or at L / 2): EDC reaches 0 inside the T20 and T30 ranges"""
    rng = np.random.RandomState(seed)
    h = (rng.randn(L) * geometric(L, 0.3, dtype=np.float64)).astype(np.float32)
    h[min(1800, L // 2):] = 0.0
    return h


def noise_tail(L, seed):
    """channel `seed % 4` of a make_rir_bank response with a diffuse tail"""
    from salsa_amd import scenes as sc
    return sc.make_rir_bank('foa', [(30, 10)], L, rt60=0.25, drr_db=6.0, seed=seed).rirs[0, seed % 4].copy()


_IMAGE_SOURCE = {}


def image_source(L, channel):
    """a channel of an image-source response from the CPU path: a 6 x 5 x 3.2 m room, beta 0.7, up to order 8 (the tail ends in exact
    zeros past the last image), generated once at 16384 taps; a shorter response is its prefix"""
    if 'h' not in _IMAGE_SOURCE:
        from salsa_amd import rooms
        room = rooms.ShoeboxRoom((6.0, 5.0, 3.2), beta=0.7)
        _IMAGE_SOURCE['h'] = rooms.room_rirs('foa', room, [(35, 15)], 1.5, 16384, max_order=8, device='cpu')[0].numpy()[0].copy()
    return _IMAGE_SOURCE['h'][channel, :L].copy()


def double_peak(L, seed):
    """a noisy decay whose largest |h| occurs twice, with opposite signs: the first index wins"""
    rng = np.random.RandomState(seed)
    h = (0.5 * rng.randn(L) * geometric(L, 0.2, dtype=np.float64)).clip(-0.9, 0.9).astype(np.float32)
    a, b = (5, 9) if L >= 10 else (0, L - 1)
    h[a], h[b] = 1.5, -1.5
    return h


FAMILIES = ('geometric', 'two_slope', 'zeros', 'impulse_first', 'impulse_last', 'decay_then_zeros', 'noise_tail', 'image_source_w',
            'double_peak', 'image_source_y', 'geometric_fast', 'noise_tail_2')


def family(name, L, seed=0):
    """one response (L) float32 of the family"""
    if name == 'geometric':
        return geometric(L, 0.2871)                 # (at T = 0.3 s the levels -5, -10, ... dB fall ON taps 600, 1200, ...: a knife edge)
    if name == 'geometric_fast':
        return geometric(L, 0.05)
    if name == 'two_slope':
        return two_slope(L, seed)
    if name == 'zeros':
        return np.zeros(L, np.float32)
    if name == 'impulse_first':
        return impulse(L, 0)
    if name == 'impulse_last':
        return impulse(L, L - 1, -0.5)
    if name == 'decay_then_zeros':
        return decay_then_zeros(L, seed)
    if name == 'noise_tail':
        return noise_tail(L, 4 + seed)
    if name == 'noise_tail_2':
        return noise_tail(L, 9 + seed)
    if name == 'image_source_w':
        return image_source(L, 0)
    if name == 'image_source_y':
        return image_source(L, 1)
    if name == 'double_peak':
        return double_peak(L, seed)
    raise KeyError(name)


def bank(L, n_rirs=3, n_channels=4, seed=0):
    """(names, h float32 (n_rirs, n_channels, L)): the families in FAMILIES' order, round and round"""
    names = [FAMILIES[i % len(FAMILIES)] for i in range(n_rirs * n_channels)]
    h = np.stack([family(name, L, seed + i) for i, name in enumerate(names)]).reshape(n_rirs, n_channels, L)
    return names, np.ascontiguousarray(h, np.float32)


# ---- shared cases and the bounds both test files hold ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(L, n_rirs=3, n_channels=4, seed=0):
    """A bank of the families with its reference, computed once and shared (never written): (names, h (R, C, L), reference params
    (R, C, 15), reference curve (R, C, L), Y (R, C, 15), kept (R, C): the knife-edge margin is above MIN_MARGIN).  At most one case
    in ten may be dropped for its margin."""
    names, h = bank(L, n_rirs, n_channels, seed)
    got = [measure_case(h[r, c]) for r in range(n_rirs) for c in range(n_channels)]
    params = np.stack([g[0]['params'] for g in got]).reshape(n_rirs, n_channels, -1)
    edc = np.stack([g[0]['edc'] for g in got]).reshape(n_rirs, n_channels, L)
    Y = np.stack([g[1] for g in got]).reshape(n_rirs, n_channels, -1)
    kept = np.array([g[2] > MIN_MARGIN for g in got]).reshape(n_rirs, n_channels)
    assert (~kept).sum() <= kept.size // 10, 'too many cases on a knife edge: %s' % [n for n, g in zip(names, got) if not g[2] > MIN_MARGIN]
    for a in (h, params, edc, Y, kept):
        a.setflags(write=False)
    return names, h, params, edc, Y, kept


def holds(what, params, edc, the_case, factor=4.0, floor=1e-12):
    """params (R, C, 15) and edc (R, C, L) or None of the code under test against the_case = case(...):
      exactly: peak, the crossings, and where every parameter is NaN or infinite (kept cases; peak in every case);
      energy and the curve within L 2^-53 relative of the correctly rounded sums -- the worst case of ANY order of adding L
        non-negative float64 terms (each of at most L - 1 additions errs by 2^-53 of a partial sum that is at most the total);
      fitted times, headrooms, DRR, C50 within factor x Y + floor x |reference|.
    -> {quantity: largest error / Y seen (inf where Y = 0 and the error is not)} for the records"""
    names, h, ref, ref_edc, Y, kept = the_case
    R, Cn, L = h.shape
    assert params.shape == ref.shape
    u = L * 2.0 ** -53
    ratios = {}
    for r in range(R):
        for c in range(Cn):
            tag = '%s %s (%d, %d) of L = %d' % (what, names[r * Cn + c], r, c, L)
            g, w = params[r, c], ref[r, c]
            assert g[IDX['peak']] == w[IDX['peak']], tag
            assert abs(g[IDX['energy']] - w[IDX['energy']]) <= u * w[IDX['energy']], tag
            if edc is not None:
                assert np.all(np.abs(edc[r, c] - ref_edc[r, c]) <= u * ref_edc[r, c]), tag
            if not kept[r, c]:
                continue
            assert np.array_equal(np.isnan(g), np.isnan(w)), '%s: NaN at %s, expected at %s' % (
                tag, [NAMES[i] for i in np.nonzero(np.isnan(g))[0]], [NAMES[i] for i in np.nonzero(np.isnan(w))[0]])
            assert np.array_equal(g == np.inf, w == np.inf) and not np.any(g == -np.inf), tag
            for name in EXACT:
                assert g[IDX[name]] == w[IDX[name]] or np.isnan(w[IDX[name]]), '%s: %s %r != %r' % (tag, name, g[IDX[name]], w[IDX[name]])
            for name in FITTED:
                i = IDX[name]
                if not np.isfinite(w[i]):
                    continue
                err = abs(g[i] - w[i])
                print('RATIO %s %s: err %.3e Y %.3e ref %.6g' % (tag, name, err, Y[r, c, i], w[i]))
                assert err <= factor * Y[r, c, i] + floor * abs(w[i]), '%s: %s off by %.3e > %g x %.3e + %g x %.6g' % (
                    tag, name, err, factor, Y[r, c, i], floor, abs(w[i]))
                ratio = err / Y[r, c, i] if Y[r, c, i] > 0 else (0.0 if err == 0 else float('inf'))
                ratios[name] = max(ratios.get(name, 0.0), ratio)
    return ratios
